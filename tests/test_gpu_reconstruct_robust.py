"""GPU tests (through the C ABI) of zk_groth16_reconstruct_robust: a batch of proofs from proof shares that are not trusted.
The five proofs are those of test_gpu_pairing._proofs (one small circuit, different r and s), on BN254 and BLS12-381 at l = 2
(n = 8).  r and s are in the clear, so the shares of A, B and C are words of dimension 2l = 4: the honest batch pins that --
at any smaller dimension the honest shares would not be codewords."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
import zksaas_amd.groth16 as zg
from test_gpu_pairing import _proofs

BOTH = ["bn254", "bls12_381"]
L, N = 2, 8
LIAR, VICTIM = 3, 2          # party 3 lies in proof 2


def _stack(shares, parties=None):
    """[(pa, pb, pc) per proof] -> (pa, pb, pc) as [nproofs][nparties][...] of the listed parties"""
    rows = list(range(N)) if parties is None else list(parties)
    return tuple(np.stack([np.asarray(sh[e])[rows] for sh in shares]) for e in range(3))


def _honest(curve):
    """(affine [5][...], bytes [5]) of zk_groth16_reconstruct, proof by proof"""
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    both = [zg.reconstruct(pp, sh) for sh in shares]
    return np.stack([a for a, _ in both]), [b for _, b in both]


def _lie(shares, elements=(0, 1, 2), liar=LIAR, victim=VICTIM, donor=4):
    """the liar's shares of `elements` of proof `victim` replaced by its shares of proof `donor`: points of the subgroup"""
    out = [tuple(np.array(x, copy=True) for x in sh) for sh in shares]
    for e in elements:
        out[victim][e][liar] = shares[donor][e][liar]
    return out


def _check_named(curve, shares, parties, elements=(0, 1, 2)):
    pp = _proofs(curve)[0]
    want_aff, want_bytes = _honest(curve)
    aff, raw, status, errpos = zg.reconstruct_robust(pp, _stack(shares, parties), parties)
    want_st = np.zeros((5, 3), dtype=np.uint8)
    want_ep = np.zeros((5, 3), dtype=np.uint32)
    for e in elements:
        want_st[VICTIM][e], want_ep[VICTIM][e] = 1, 1 << LIAR
    assert np.array_equal(status, want_st) and np.array_equal(errpos, want_ep)
    assert np.array_equal(aff, want_aff) and raw == want_bytes


@pytest.mark.parametrize("curve", BOTH)
def test_honest_proofs_equal_reconstruct_and_verify(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    want_aff, want_bytes = _honest(curve)
    aff, raw, status, errpos = zg.reconstruct_robust(pp, _stack(shares))
    assert not status.any() and not errpos.any()
    assert np.array_equal(aff, want_aff) and raw == want_bytes
    assert zg.verify(pp, pvk, list(aff), [[w[1]]] * 5) == [True] * 5
    # affine only
    aff2, none, status2, _ = zg.reconstruct_robust(pp, _stack(shares), want_bytes=False)
    assert none is None and np.array_equal(aff2, want_aff) and not status2.any()


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("absent", [(), (6,), (0, 5)], ids=["all", "one_absent", "2l-2_absent"])
def test_one_liar_is_corrected_and_named(curve, absent):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    assert len(absent) <= 2 * L - 2
    parties = None if not absent else [q for q in range(N) if q not in absent]
    _check_named(curve, _lie(shares), parties)


@pytest.mark.parametrize("curve", BOTH)
def test_a_liar_in_c_only(curve):
    shares = _proofs(curve)[5]
    _check_named(curve, _lie(shares, elements=(2,)), None, elements=(2,))


@pytest.mark.parametrize("curve", BOTH)
def test_a_share_off_the_curve_is_corrected_and_named(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    bad = [tuple(np.array(x, copy=True) for x in sh) for sh in shares]
    nl = pp.fq.nl
    a = bad[VICTIM][0][LIAR]
    a[nl:2 * nl] = a[:nl]                      # Y := X: (X, X, Z) is on the curve for no share here
    b = bad[VICTIM][1][LIAR]
    b[2 * nl:4 * nl] = b[:2 * nl]
    _check_named(curve, bad, None, elements=(0, 1))


@pytest.mark.parametrize("curve", BOTH)
def test_two_liars_in_a_fail_that_element_only(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    want_aff, want_bytes = _honest(curve)
    bad = _lie(_lie(shares, elements=(0,)), elements=(0,), liar=6)
    aff, raw, status, errpos = zg.reconstruct_robust(pp, _stack(bad))
    want_st = np.zeros((5, 3), dtype=np.uint8)
    want_st[VICTIM][0] = 2
    assert np.array_equal(status, want_st) and not errpos.any()
    nl = pp.fq.nl
    assert not aff[VICTIM][:2 * nl].any()                                   # the failed element is (0, 0)
    assert np.array_equal(aff[VICTIM][2 * nl:], want_aff[VICTIM][2 * nl:])  # B and C of that proof are still decoded
    assert raw[VICTIM] == bytes(4 * pp.fq.nbytes)
    for i in range(5):
        if i != VICTIM:
            assert np.array_equal(aff[i], want_aff[i]) and raw[i] == want_bytes[i]


@pytest.mark.parametrize("curve", BOTH)
def test_2l_plus_1_parties_detect_only_and_2l_is_refused(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    want_aff, want_bytes = _honest(curve)
    parties = [0, 2, 3, 5, 7]
    assert len(parties) == 2 * L + 1 and LIAR in parties
    aff, raw, status, errpos = zg.reconstruct_robust(pp, _stack(shares, parties), parties)
    assert not status.any() and np.array_equal(aff, want_aff) and raw == want_bytes
    aff, raw, status, errpos = zg.reconstruct_robust(pp, _stack(_lie(shares), parties), parties)
    want_st = np.zeros((5, 3), dtype=np.uint8)
    want_st[VICTIM] = 2
    assert np.array_equal(status, want_st) and not errpos.any()
    assert not aff[VICTIM].any() and raw[VICTIM] == bytes(4 * pp.fq.nbytes)
    few = parties[:2 * L]
    with pytest.raises(zk.ZkError) as e:
        zg.reconstruct_robust(pp, _stack(shares, few), few)
    assert e.value.code == 2                   # ZK_ERR_PROTOCOL
    # the refusals leave the context usable
    pa, pb, pc = _stack(shares)
    st = np.zeros((5, 3), dtype=np.uint8)
    lib, u32 = pp.lib, C.c_uint32
    args = lambda ids, cnt, status: (pp.h, 5, pa.ctypes.data, pb.ctypes.data, pc.ctypes.data, ids, cnt, None, None, status,
                                     None, None)
    assert lib.zk_groth16_reconstruct_robust(*args((u32 * 5)(0, 2, 2, 5, 7), 5, st.ctypes.data)) == 4
    assert lib.zk_groth16_reconstruct_robust(*args((u32 * 5)(0, 2, 3, 5, 8), 5, st.ctypes.data)) == 4
    assert lib.zk_groth16_reconstruct_robust(*args(None, N + 1, st.ctypes.data)) == 4
    assert lib.zk_groth16_reconstruct_robust(*args(None, N, None)) == 4
    assert lib.zk_groth16_reconstruct_robust(pp.h, 0, None, None, None, None, N, None, None, st.ctypes.data, None, None) == 0
    aff, raw, status, errpos = zg.reconstruct_robust(pp, _stack(shares))
    assert not status.any() and np.array_equal(aff, want_aff)
