"""zk_groth16_verify_bytes and zk_groth16_verify_all_bytes on the device (`pytest -m gpu`): proofs as
`Proof::serialize_compressed` bytes and public inputs as canonical Fr bytes, against zk_groth16_verify on the decoded points
and against single defects placed in otherwise good batches.  Verdicts are bytes: every comparison is exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from zksaas_amd import groth16 as zg, wire
from zksaas_amd.api import ZK_G1, ZK_G2, DeviceBuffer
from oracle.curve import g1, g2
from oracle.params import CURVES

import subgroup_points as sp
from gpu_util import ctx
from test_gpu_pairing import _decode_proof, _proofs
from test_gpu_verify_all import SEED, DlBatch

BOTH = ["bn254", "bls12_381"]
NB = 33
SPOTS = (0, 16, 32)


def fr_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def rows_to_bytes(pp, rows):
    """[count][8 nl] affine rows A | B | C -> list of Proof::serialize_compressed byte strings (zk_points_compress)"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    n, nl, nb = rows.shape[0], pp.fq.nl, pp.fq.nbytes
    col = lambda lo, hi, grp: wire.points_to_bytes(pp, grp, DeviceBuffer.from_numpy(pp, np.ascontiguousarray(rows[:, lo:hi])), n)
    a, b, c = col(0, 2 * nl, ZK_G1), col(2 * nl, 6 * nl, ZK_G2), col(6 * nl, 8 * nl, ZK_G1)
    return [a[i * nb:(i + 1) * nb] + b[2 * i * nb:2 * (i + 1) * nb] + c[i * nb:(i + 1) * nb] for i in range(n)]


# ------------------------------------------------------------------------------------------------------------ real proofs
@pytest.mark.parametrize("curve", BOTH)
def test_real_proofs_from_their_bytes(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    recon = [zg.reconstruct(pp, sh) for sh in shares]
    assert all(np.array_equal(a, b) for (a, _), b in zip(recon, affs))
    raw = [b for _, b in recon]
    assert all(len(b) == 4 * pp.fq.nbytes for b in raw)
    assert rows_to_bytes(pp, np.stack(affs)) == raw                    # (the helper the other tests build their bytes with)
    for count in (0, 1, 3, 65):
        pb = [raw[i % 5] for i in range(count)]
        pa = [affs[i % 5] for i in range(count)]
        xs_int = [[w[1]]] * count
        got = zg.verify_bytes(pp, pvk, pb, [fr_bytes(x) for x in xs_int])
        want = zg.verify(pp, pvk, pa, xs_int) if count else []
        assert got == want == [True] * count, count
        assert zg.verify_all_bytes(pp, pvk, pb, [fr_bytes(x) for x in xs_int], seed=SEED) is True, count
    # a wrong input value fails as it does from the points
    assert zg.verify_bytes(pp, pvk, raw[:2], [fr_bytes([w[1]]), fr_bytes([(w[1] + 1) % c.r])]) == [True, False]


# ------------------------------------------------------------------------------------- one defect in a good batch of 33
@functools.lru_cache(maxsize=None)
def _batch(curve):
    dl = DlBatch(curve, 2, NB, 40)
    pp = dl.pp
    pb = rows_to_bytes(pp, dl.good)
    xb = [fr_bytes(x) for x in dl.xs]
    assert zg.verify(pp, dl.pvk, dl.good, dl.xs) == [True] * NB
    return dl, pb, xb


def _expect_one_bad(dl, pb, xb, at, what):
    pp = dl.pp
    assert zg.verify_bytes(pp, dl.pvk, pb, xb) == [i != at for i in range(NB)], (what, at)       # (returns: the call succeeds)
    assert zg.verify_all_bytes(pp, dl.pvk, pb, xb, seed=SEED) is False, (what, at)


def _off_curve_encoding(pp, curve, enc, g2=False):
    for k in range(1, 200):
        b = bytearray(enc)
        b[len(enc) // 2 - 1] ^= k
        try:
            wire.point_from_bytes(pp, bytes(b), g2, curve)
        except ValueError as e:
            if "not on the curve" in str(e):
                return bytes(b)
    raise AssertionError("no x off the curve found")


@pytest.mark.parametrize("curve", BOTH)
def test_a_good_batch_is_accepted_and_its_value_is_one(curve):
    dl, pb, xb = _batch(curve)
    pp = dl.pp
    assert zg.verify_bytes(pp, dl.pvk, pb, xb) == [True] * NB
    ok, gt = zg.verify_all_bytes(pp, dl.pvk, pb, xb, seed=SEED, want_gt=True)
    assert ok is True and gt == [1] + [0] * 11


@pytest.mark.parametrize("at", SPOTS)
@pytest.mark.parametrize("curve", BOTH)
def test_an_a_that_does_not_decode(curve, at):
    dl, pb, xb = _batch(curve)
    n = dl.pp.fq.nbytes
    bad = list(pb)
    bad[at] = _off_curve_encoding(dl.pp, curve, pb[at][:n]) + pb[at][n:]
    _expect_one_bad(dl, bad, xb, at, "A off the curve")


@pytest.mark.parametrize("at", SPOTS)
def test_b_with_its_compression_flag_cleared_on_bls12_381(at):
    dl, pb, xb = _batch("bls12_381")
    n = dl.pp.fq.nbytes
    b = bytearray(pb[at])
    assert b[n] & 0x80
    b[n] &= 0x7F
    bad = list(pb)
    bad[at] = bytes(b)
    _expect_one_bad(dl, bad, xb, at, "B without the compression flag")


@pytest.mark.parametrize("at", SPOTS)
@pytest.mark.parametrize("curve", BOTH)
def test_an_input_that_is_not_below_r(curve, at):
    dl, pb, xb = _batch(curve)
    r = CURVES[curve].r
    for what, enc in (("input = r", int(r).to_bytes(32, "little")), ("top byte 0xFF", xb[at][32:63] + b"\xff")):
        bad = list(xb)
        bad[at] = xb[at][:32] + enc                                   # the second input of the proof
        _expect_one_bad(dl, pb, bad, at, what)
    bad = list(xb)
    bad[at] = int(r).to_bytes(32, "little") + xb[at][32:]             # ... and the first
    _expect_one_bad(dl, pb, bad, at, "first input = r")


@pytest.mark.parametrize("at", SPOTS)
@pytest.mark.parametrize("curve", BOTH)
def test_c_replaced_by_another_subgroup_point(curve, at):
    dl, pb, xb = _batch(curve)
    n = dl.pp.fq.nbytes
    bad = list(pb)
    bad[at] = pb[at][:3 * n] + pb[(at + 1) % NB][3 * n:]
    _expect_one_bad(dl, bad, xb, at, "C of the neighbour")


@pytest.mark.parametrize("at", SPOTS)
@pytest.mark.parametrize("curve", BOTH)
def test_b_moved_out_of_the_subgroup_by_a_torsion_point(curve, at):
    dl, pb, xb = _batch(curve)
    pp, n = dl.pp, dl.pp.fq.nbytes
    G = g2(CURVES[curve])
    t2 = sp.classes(curve, 2)["torsion"][0][0]
    B = _decode_proof(pp, dl.good[at])[1]
    moved = G.to_affine(G.add(G.from_affine(B), G.from_affine(t2)))
    assert G.on_curve(moved) and not sp.in_subgroup(G, moved)
    bad = list(pb)
    bad[at] = pb[at][:n] + wire.point_to_bytes(pp, moved, True, curve) + pb[at][3 * n:]
    _expect_one_bad(dl, bad, xb, at, "B + T2")


@pytest.mark.parametrize("at", SPOTS)
def test_a_moved_out_of_the_subgroup_by_a_torsion_point_on_bls12_381(at):
    curve = "bls12_381"
    dl, pb, xb = _batch(curve)
    pp, n = dl.pp, dl.pp.fq.nbytes
    G = g1(CURVES[curve])
    t1 = sp.classes(curve, 1)["torsion"][1][0]
    A = _decode_proof(pp, dl.good[at])[0]
    moved = G.to_affine(G.add(G.from_affine(A), G.from_affine(t1)))
    assert G.on_curve(moved) and not sp.in_subgroup(G, moved)
    bad = list(pb)
    bad[at] = wire.point_to_bytes(pp, moved, False, curve) + pb[at][n:]
    _expect_one_bad(dl, bad, xb, at, "A + T1")


# --------------------------------------------------------------------------------------------------------- one workspace
@pytest.mark.parametrize("curve", BOTH)
def test_calls_of_different_sizes_share_the_workspace(curve):
    dl, pb, xb = _batch(curve)
    pp = dl.pp
    n = pp.fq.nbytes
    bad = list(pb)
    bad[2] = pb[2][:3 * n] + pb[3][3 * n:]
    assert zg.verify_bytes(pp, dl.pvk, bad, xb) == [i != 2 for i in range(NB)]
    assert zg.verify_bytes(pp, dl.pvk, bad[:3], xb[:3]) == [True, True, False]
    assert zg.verify_all_bytes(pp, dl.pvk, pb, xb, seed=SEED) is True
    assert zg.verify_all_bytes(pp, dl.pvk, bad[:3], xb[:3], seed=SEED) is False
    rows = dl.good.copy()
    nl = pp.fq.nl
    rows[1, 6 * nl:] = dl.good[0, 6 * nl:]
    assert zg.verify(pp, dl.pvk, rows[:4], dl.xs[:4]) == [True, False, True, True]      # the plain call after a bytes call
    assert zg.verify_all(pp, dl.pvk, dl.good, dl.xs, seed=SEED) is True
