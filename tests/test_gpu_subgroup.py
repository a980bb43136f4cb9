"""zk_points_subgroup_check and zk_points_decompress_checked on the device (`pytest -m gpu`) against the ground truth
"[r]P = O" of the oracle's group law (tests/subgroup_points.py) and against zk_points_decompress.  Everything is an integer
or a byte: every comparison is exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import groth16 as zg, wire
from zksaas_amd.api import ZK_G1, ZK_G2, DeviceBuffer, points_decompress_checked, points_subgroup_check
from oracle.params import CURVES

import subgroup_points as sp
from gpu_util import ctx, enc_affine

BOTH = ["bn254", "bls12_381"]
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 300)
RUN = (70, 134)                  # a run of 64 bad points between good ones (where the vector is long enough)


def raw_row(pp, vals):
    """plain integers -> uint64 limbs, unconverted (for coordinates that are not below q)"""
    mask = (1 << 64) - 1
    return np.array([(v >> (64 * k)) & mask for v in vals for k in range(pp.fq.nl)], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def pools(curve, grp):
    """(good rows, bad rows): Montgomery limb rows by ground truth, every class of subgroup_points among them"""
    pp = ctx(curve)
    q = CURVES[curve].q
    good, bad = [], []
    for name, pts in sp.classes(curve, grp).items():
        for p, ok in pts:
            (good if ok else bad).append(enc_affine(pp, [p], grp == 2)[0])
    bad.append(enc_affine(pp, [sp.off_curve(curve, grp)], grp == 2)[0])
    mont = [c * pp.fq.R % q for c in sp.flat(sp.group(curve, grp).gen, grp)]
    nc = 2 * grp
    for k in range(nc):                                   # the generator with one coordinate lifted by q; q and q + 1 themselves
        bad.append(raw_row(pp, [c + q if j == k else c for j, c in enumerate(mont)]))
        bad.append(raw_row(pp, [q if j == k else 0 for j in range(nc)]))
        bad.append(raw_row(pp, [q + 1 if j == k else c for j, c in enumerate(mont)]))
    assert len(good) >= 18 and len(bad) >= 7
    return good, bad


def layout(n):
    """is element i good?  Good and bad alternate, a run of 64 bad ones sits between good ones, the last element is bad."""
    want = [i % 2 == 0 for i in range(n)]
    if n > RUN[1] + 1:
        for i in range(*RUN):
            want[i] = False
        want[RUN[0] - 1] = want[RUN[1]] = True
    if n:
        want[-1] = False
    return want


@pytest.mark.parametrize("grp", [1, 2])
@pytest.mark.parametrize("curve", BOTH)
def test_subgroup_check_equals_the_ground_truth_in_mixed_waves(curve, grp):
    pp = ctx(curve)
    good, bad = pools(curve, grp)
    group = ZK_G2 if grp == 2 else ZK_G1
    for n in LENGTHS:
        want = layout(n)
        gi = bi = 0
        rows = []
        for w in want:
            if w:
                rows.append(good[gi % len(good)])
                gi += 1
            else:
                rows.append(bad[bi % len(bad)])
                bi += 1
        if n == 300:
            assert gi >= len(good) and bi >= len(bad)       # every class was in the vector
        buf = DeviceBuffer.from_numpy(pp, np.stack(rows)) if n else DeviceBuffer(pp, 16)
        got = points_subgroup_check(pp, group, buf, n)
        assert got.tolist() == [int(w) for w in want], (curve, grp, n)


# --------------------------------------------------------------------------------------------- decompress_checked
def _size(pp, grp):
    return pp.fq.nbytes * grp


@functools.lru_cache(maxsize=None)
def _subgroup_bytes(curve, grp):
    """130 subgroup points (the identity among them) and their compressed encodings"""
    pp = ctx(curve)
    group = ZK_G2 if grp == 2 else ZK_G1
    c = CURVES[curve]
    ks = [(7 * i * i + 3) % c.r for i in range(130)]
    ks[5] = 0
    pts = zg.base_points(pp, group, pp.upload_fr(ks), 130)
    data = wire.points_to_bytes(pp, group, pts, 130)
    return pts.to_numpy().reshape(130, -1), data


def _defects(curve, grp, enc):
    """name -> the encoding `enc` of a non-identity point with that defect"""
    pp = ctx(curve)
    q, n, zc = CURVES[curve].q, pp.fq.nbytes, curve in wire.ZCASH_CURVES
    size = n * grp
    out = {}
    flag = 0 if zc else size - 1                           # the byte that carries the flags
    if zc:
        b = bytearray(enc)
        b[0] &= 0x7F
        out["flag_missing"] = bytes(b)                     # (ark-ec's default encoding has no compression flag)
    b = bytearray(enc)
    b[flag] |= (0x40 | 0x20) if zc else 0xC0
    out["both_flags"] = bytes(b)
    # x >= q: the coordinate that shares its bytes with the flags keeps its value, the other one (G2) or it (G1) becomes q
    b = bytearray(enc)
    qb = q.to_bytes(n, "big" if zc else "little")
    if grp == 1:
        keep = b[flag] & (0xE0 if zc else 0xC0)
        b[:] = qb
        b[flag] |= keep
    elif zc:
        b[n:] = qb                                         # c0 (zcash: c1 || c0)
    else:
        b[:n] = qb                                         # c0 (c0 || c1)
    out["x_not_below_q"] = bytes(b)
    for k in range(1, 200):                                # an x with no y on the curve
        b = bytearray(enc)
        b[size // 2 - 1] ^= k
        try:
            wire.point_from_bytes(pp, bytes(b), grp == 2, curve)
        except ValueError as e:
            if "not on the curve" in str(e):
                out["x_off_curve"] = bytes(b)
                break
    b = bytearray(size)
    b[flag] = 0xC0 if zc else 0x40
    b[size // 2] = 1
    out["infinity_nonzero_x"] = bytes(b)
    assert len(out) == (5 if zc else 4)
    for v in out.values():                                 # each is what the existing decompression rejects
        with pytest.raises(ValueError):
            wire.point_from_bytes(pp, v, grp == 2, curve)
    return out


@pytest.mark.parametrize("grp", [1, 2])
@pytest.mark.parametrize("curve", BOTH)
def test_decompress_checked_on_valid_encodings_equals_decompress(curve, grp):
    pp = ctx(curve)
    group = ZK_G2 if grp == 2 else ZK_G1
    rows, data = _subgroup_bytes(curve, grp)
    plain, count = wire.points_from_bytes(pp, group, data)
    out, count2, ok = wire.points_from_bytes_checked(pp, group, data)
    assert count == count2 == 130 and ok.tolist() == [1] * 130
    assert np.array_equal(out.to_numpy().reshape(130, -1), rows)
    assert np.array_equal(out.to_numpy(), plain.to_numpy())
    out2, _, ok2 = wire.points_from_bytes_checked(pp, group, data)              # determinism
    assert out2.to_numpy().tobytes() == out.to_numpy().tobytes() and ok2.tobytes() == ok.tobytes()
    raw = DeviceBuffer.from_numpy(pp, np.frombuffer(data, dtype=np.uint8))
    _, ok0 = points_decompress_checked(pp, group, raw, 0)                       # len = 0 launches nothing
    assert ok0.size == 0


@pytest.mark.parametrize("grp", [1, 2])
@pytest.mark.parametrize("curve", BOTH)
def test_decompress_checked_one_defect_fails_that_element_only(curve, grp):
    pp = ctx(curve)
    group = ZK_G2 if grp == 2 else ZK_G1
    rows, data = _subgroup_bytes(curve, grp)
    size = _size(pp, grp)
    for name, enc in _defects(curve, grp, data[size:2 * size]).items():
        for at in (0, 64, 129):
            bad = bytearray(data)
            bad[at * size:(at + 1) * size] = enc
            out, count, ok = wire.points_from_bytes_checked(pp, group, bytes(bad))     # (returns: the call succeeds)
            assert ok.tolist() == [int(i != at) for i in range(130)], (name, at)
            got = out.to_numpy().reshape(130, -1)
            assert not got[at].any(), (name, at)
            keep = [i for i in range(130) if i != at]
            assert np.array_equal(got[keep], rows[keep]), (name, at)


@pytest.mark.parametrize("curve,grp", [("bn254", 2), ("bls12_381", 1), ("bls12_381", 2)])
def test_decompress_checked_keeps_a_point_outside_the_subgroup(curve, grp):
    pp = ctx(curve)
    group = ZK_G2 if grp == 2 else ZK_G1
    rows, data = _subgroup_bytes(curve, grp)
    size = _size(pp, grp)
    cl = sp.classes(curve, grp)
    for at, (p, truth) in zip((0, 64, 129), cl["gen_plus_torsion"] + cl["torsion"] + cl["curve"]):
        assert not truth
        bad = bytearray(data)
        bad[at * size:(at + 1) * size] = wire.point_to_bytes(pp, p, grp == 2, curve)
        out, count, ok = wire.points_from_bytes_checked(pp, group, bytes(bad))
        assert ok.tolist() == [int(i != at) for i in range(130)], at
        want = rows.copy()
        want[at] = enc_affine(pp, [p], grp == 2)[0]
        assert np.array_equal(out.to_numpy().reshape(130, -1), want), at


def test_bls12_377_context_is_bad_input_from_all_five_calls():
    pp = ctx("bls12_377")
    buf = DeviceBuffer(pp, 4096)
    pvk = type("V", (), {"h": None, "n_abc": 2})()
    calls = (lambda: points_subgroup_check(pp, ZK_G1, buf, 1), lambda: points_decompress_checked(pp, ZK_G1, buf, 1),
             lambda: wire.points_from_bytes_checked(pp, ZK_G1, bytes(48)),
             lambda: zg.verify_bytes(pp, pvk, bytes(4 * pp.fq.nbytes), bytes(32)),
             lambda: zg.verify_all_bytes(pp, pvk, bytes(4 * pp.fq.nbytes), bytes(32)))
    for call in calls:
        with pytest.raises(zk.ZkError) as e:
            call()
        assert e.value.code == 4 and "no pairing parameters" in e.value.msg
