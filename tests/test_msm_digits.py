"""The scalar construction of tests/msm_digits.py does what the GPU tests rely on (no GPU needed): the recoding of every
engineered scalar is exactly the chosen digits, every freely chosen window receives every digit of (-half, +half] \\ {0}
(+half, the largest bucket, included), and the numpy forms agree with the plain-integer ones."""
import numpy as np
import pytest

import msm_digits as md
from oracle.params import CURVES

CURVE_NAMES = ("bn254", "bls12_381", "bls12_377")


def test_geometry_by_hand():
    r = CURVES["bn254"].r                                  # 254 bits: T = 255
    g = md.geometry(r, 13)
    assert (g.T, g.nwin, g.c, g.wide, g.B) == (255, 20, 13, 15, 4096)
    assert g.widths == (13,) * 15 + (12,) * 5 and g.starts[15] == 195 and g.starts[-1] == 243
    g = md.geometry(r, 14)
    assert (g.nwin, g.c, g.wide) == (19, 14, 8)
    g = md.geometry(r, 2)
    assert (g.nwin, g.c, g.wide, g.widths[-1]) == (128, 2, 127, 1)
    g = md.geometry(r, 20)
    assert (g.nwin, g.c, g.wide, g.B) == (13, 20, 8, 1 << 19)
    g = md.geometry(r, 17, table=True)                     # re-rounded: 17 bits asked = 15 windows of 17
    assert (g.nwin, g.c, g.wide) == (15, 17, 15)
    r = CURVES["bls12_381"].r                              # 255 bits: T = 256
    g = md.geometry(r, 16)
    assert (g.nwin, g.c, g.wide) == (16, 16, 16)
    g = md.geometry(r, 3)
    assert (g.nwin, g.c, g.wide) == (86, 3, 84)
    assert md.geometry(CURVES["bls12_377"].r, 12)[3:6] == (22, 12, 12)     # 253 bits: T = 254


def test_recode_by_hand():
    g = md.geometry(CURVES["bn254"].r, 13)                 # half = 4096 in window 0
    z = [0] * 19
    assert md.recode(4096, g) == [4096] + z                # +half stays positive: bucket k = half
    assert md.recode(4097, g) == [-4095, 1] + z[1:]        # half + 1 -> -(half - 1) and a carry
    assert md.recode(8191, g) == [-1, 1] + z[1:]
    assert md.recode((1 << 26) - 1, g) == [-1, 0, 1] + z[2:]   # the carry runs through a window of all ones
    assert md.nonzero_digits(0, g) == 0 and md.nonzero_digits((1 << 26) - 1, g) == 2


def _check_width(r, g, indices):
    """recoder == construction and numpy == plain integers on `indices`; coverage over ALL 2B scalars (numpy)."""
    full = md.engineered_digit_array(r, g)
    assert full.shape == (2 * g.B, g.nwin)
    for w in range(md.free_windows(r, g)):
        h = md.half(g, w)
        seen = np.unique(full[:, w])
        want = np.array([d for d in range(-h + 1, h + 1) if d], dtype=np.int64)
        assert np.array_equal(seen, want), (g.c_req, w)
    assert (full[:, :-1] != 0).all()                       # every window below the top one costs an addition
    nl = (g.bits + 63) // 64
    idx = list(indices)
    sc = md.engineered(r, g, idx)
    limbs = md.digits_to_limbs(full[idx], g, nl)
    assert md.limbs_to_ints(limbs) == sc
    for i, s in zip(idx, sc):
        assert 0 < s < r
        ds = md.engineered_digits(i, r, g)
        assert md.recode(s, g) == ds == list(full[i]), (g.c_req, i)
        assert md.nonzero_digits(s, g) == sum(1 for d in ds if d)


@pytest.mark.parametrize("c_req", range(2, 15))
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_engineered_scalars_recode_to_their_digits(curve, c_req):
    r = CURVES[curve].r
    g = md.geometry(r, c_req)
    _check_width(r, g, range(2 * g.B))


@pytest.mark.parametrize("c_req", range(15, 21))
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_engineered_scalars_wide_windows(curve, c_req):
    """15..20 bits: coverage over all 2B scalars, recoder == construction on a strided subset and at both ends."""
    r = CURVES[curve].r
    g = md.geometry(r, c_req)
    n = 2 * g.B
    _check_width(r, g, sorted(set(range(0, n, n // 4096 + 1)) | set(range(64)) | set(range(n - 64, n))))


@pytest.mark.parametrize("c_req", range(8, 23))
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_table_geometries(curve, c_req):
    """Fixed-base tables (msm_table_c 8..22): same digits; above 16 bits the GPU tests run 2^16 chosen scalars, which
    must reach the magnitudes half_w, half_w - 1, 1 and 2 in every freely chosen window, both signs where there are
    two (so k = B in every c-bit window and k = B/2 in every narrow one)."""
    r = CURVES[curve].r
    g = md.geometry(r, c_req, table=True)
    n = 2 * g.B
    if g.c <= 16:
        assert md.table_indices(g) == list(range(n))
        _check_width(r, g, sorted(set(range(0, n, n // 2048 + 1)) | set(range(n - 64, n))))
        return
    idx = md.table_indices(g)
    assert len(idx) == 1 << 16 == len(set(idx)) and 0 <= idx[0] and idx[-1] < n
    digs = md.engineered_digit_array(r, g, idx)
    for w in range(md.free_windows(r, g)):
        h = md.half(g, w)
        seen = set(np.unique(digs[:, w]).tolist())
        assert {h, h - 1, -(h - 1), 1, -1, 2, -2} <= seen, (c_req, w)
    sub = idx[:: len(idx) // 1024]
    assert md.limbs_to_ints(md.digits_to_limbs(digs[:: len(idx) // 1024], g, (g.bits + 63) // 64)) == md.engineered(r, g, sub)
    for i, s in zip(sub, md.engineered(r, g, sub)):
        assert 0 < s < r and md.recode(s, g) == md.engineered_digits(i, r, g)


@pytest.mark.parametrize("c_req", (2, 3, 7, 8, 12, 13, 16, 19, 20, 22))
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_edge_scalars(curve, c_req):
    r = CURVES[curve].r
    g = md.geometry(r, c_req)
    edges = md.edge_scalars(r, g)
    assert len(set(edges)) >= 3 * (g.bits - 1)
    assert {0, 1, r - 1, (r - 1) // 2, (1 << (g.bits - 1)) - 1, 1 << (g.bits - 1)} <= set(edges)
    for s in edges:
        assert 0 <= s < r
        ds = md.recode(s, g)
        assert md.compose(ds, g) == s
        assert all(-md.half(g, w) < d <= md.half(g, w) for w, d in enumerate(ds))
    for w in range(g.nwin):
        h, st = md.half(g, w), g.starts[w]
        if (h << st) < r:
            assert (h << st) in edges
            assert md.recode(h << st, g) == [0] * w + [h] + [0] * (g.nwin - 1 - w)
        if ((h + 1) << st) < r and h > 1:
            assert ((h + 1) << st) in edges
            assert md.recode((h + 1) << st, g) == [0] * w + [-(h - 1), 1] + [0] * (g.nwin - 2 - w)
    hs = md.half_digit_scalar(r, g)
    assert hs in edges and hs < r
    assert md.recode(hs, g)[:-1] == [md.half(g, w) for w in range(g.nwin - 1)]
    nl = (g.bits + 63) // 64
    assert md.limbs_to_ints(md.ints_to_limbs(edges, nl)) == edges


def test_montgomery_and_aggregate():
    r = CURVES["bn254"].r
    g = md.geometry(r, 9)
    sc = md.engineered(r, g) + md.edge_scalars(r, g)
    limbs = md.ints_to_limbs(sc, 4)
    assert md.limbs_to_ints(md.montgomery_limbs(limbs, r)) == [(s << 256) % r for s in sc]
    i = np.arange(len(sc))
    cls, live = i % 48, (i != 5) & (i % 11 != 3)
    want = [0] * 48
    for k, s in enumerate(sc):
        if k != 5 and k % 11 != 3:
            want[k % 48] = (want[k % 48] + s) % r
    assert md.aggregate(limbs, cls, 48, live, r) == want
