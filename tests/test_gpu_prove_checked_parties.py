"""GPU tests (through the C ABI) for zk_groth16_prove_checked_parties: the checked prover with a party list carried through
the whole proof -- the h chain of zk_circom_h_checked_parties and the list's coefficients in the five MSM rounds and the host
in-mask terms.  The setting of test_gpu_prove_checked.py: its small circuit, bn254 at l = 2, all twelve masks; party 5 absent.
  (a) honest input    the proof reconstructs to the scalars og.verify_scalars accepted and equals the honest proof as group
                      elements per party; items 0..5 clean, item 6 the all-zero "not checked" row
  (b) poisoned input  party 5's rows of qap_*, a_share, ax_share and of the fft / degred in-masks replaced by random field
                      elements, its MSM in-mask points by other valid points: the same proof as (a), and it verifies.  On that
                      input zk_groth16_prove_checked with all parties does not verify (the MSM rounds read the liar), nor does
                      the unchecked prover
  (c) no state        a plain prove afterwards gives the proof it gave before
  (d) all n parties   the proof and the report of the check=True call"""
import ctypes as C
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import groth16 as zg

from test_gpu_prove_checked import _clean, _same_proof, _setting, _verifies

ABSENT = 5
BAD_INPUT, PROTOCOL = 4, 2


def _raw(rng, *shape):
    a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


def _poison_rows(pp, buf, rng, p):
    rows = buf.to_numpy().reshape(pp.n, -1, 4).copy()
    rows[p] = _raw(rng, rows.shape[1])
    return zk.DeviceBuffer.from_numpy(pp, rows)


def _poisoned(S, p):
    """party p's rows of every input and in-mask replaced -> (witness, masks struct, what must stay alive)"""
    pp = S.pp
    rng = np.random.default_rng(710)
    qap = [_poison_rows(pp, q, rng, p) for q in S.wit.qap]
    wit = types.SimpleNamespace(qap=qap, a_share=_poison_rows(pp, S.wit.a_share, rng, p),
                                ax_share=_poison_rows(pp, S.wit.ax_share, rng, p), log_m=S.wit.log_m, len_a=S.wit.len_a,
                                len_w=S.wit.len_w)
    mk = zg.Masks()
    C.memmove(C.byref(mk), C.byref(S.masks.ct), C.sizeof(zg.Masks))
    keep = []
    for k in range(6):
        keep.append(_poison_rows(pp, S.masks.fft[k].in_mask, rng, p))
        mk.fft_in[k] = keep[-1].ptr
    keep.append(_poison_rows(pp, S.masks.degred.in_mask, rng, p))
    mk.degred_in = keep[-1].ptr
    for k in range(5):
        pts = S.masks.msm[k].in_mask.copy()
        pts[p] = pts[(p + 3) % pp.n]                 # another valid point of the same group
        assert not np.array_equal(pts[p], S.masks.msm[k].in_mask[p])
        keep.append(pts)
        mk.msm_in[k] = pts.ctypes.data
    return wit, mk, keep


def _unchecked_item_6(pp, rep, Lc):
    st, ep = rep.status_host().reshape(7, Lc), rep.errpos_host().reshape(7, Lc)
    return not st.any() and not ep.any() and rep.summaries == [_clean(pp, Lc)] * 6 + [[0] * (3 + pp.n)]


def test_honest_and_poisoned_proofs_of_n_minus_1_parties_are_the_honest_proof():
    S = _setting()
    pp, Lc = S.pp, (1 << S.wit.log_m) // S.pp.l
    parties = [p for p in range(pp.n) if p != ABSENT]
    # (a)
    proof, rep = zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13, check=True, parties=parties)
    assert rep.parties == parties
    assert _verifies(S, proof) and _same_proof(pp, proof, S.honest)
    assert _unchecked_item_6(pp, rep, Lc)
    # (b)
    wit, mk, keep = _poisoned(S, ABSENT)
    again, rep = zg.prove(pp, S.crs, wit, S.r, S.s, masks=mk, seed=13, check=True, parties=parties)
    assert _verifies(S, again) and _same_proof(pp, again, proof)
    assert _unchecked_item_6(pp, rep, Lc)
    # the input bites: the MSM rounds of the all-parties checked prover read the liar, and so does the unchecked prover
    full, full_rep = zg.prove(pp, S.crs, wit, S.r, S.s, masks=mk, seed=13, check=True)
    assert not _verifies(S, full)
    assert (full_rep.errpos_host().reshape(7, Lc)[:6] == 1 << ABSENT).all()
    assert not _verifies(S, zg.prove(pp, S.crs, wit, S.r, S.s, masks=mk, seed=13))
    # (c) no state is left behind
    assert _same_proof(pp, zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13), S.honest)
    del keep


def test_all_parties_listed_is_the_checked_prover():
    S = _setting()
    pp = S.pp
    want, ref = zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13, check=True)
    got, rep = zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13, check=True, parties=list(range(pp.n)))
    assert _same_proof(pp, got, want) and _verifies(S, got)
    for a, b in ((rep.status, ref.status), (rep.errpos, ref.errpos), (rep.summary_d, ref.summary_d)):
        assert np.array_equal(a.to_numpy(np.uint8), b.to_numpy(np.uint8))


def test_refusals():
    S = _setting()
    pp = S.pp
    for parties, code in (([0, 1, 2, 3, 4, 5], PROTOCOL), ([0, 1, 3, 2, 4, 5, 6], BAD_INPUT), ([0, 1, 2, 3, 4, 5, 8], BAD_INPUT)):
        with pytest.raises(zk.ZkError) as err:
            zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13, check=True, parties=parties)
        assert err.value.code == code, parties
    with pytest.raises(ValueError):
        zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13, parties=list(range(pp.n - 1)))
    assert _same_proof(pp, zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13), S.honest)
