"""GPU parity (through the C ABI) for zk_pss_unpack_points_robust, zk_pss_repair_points and zk_d_msm_checked.  A word of point
shares is the lift of a scalar word with zk_base_mul, Y_p = y_p G, so every expected verdict comes from the scalars:
tests/points_robust_model.py (the unchanged tests/gao_model.py cut down to one error per chunk), and every expected point is
zk_base_mul of a scalar -- affine output is canonical, so points are compared as bytes.  Vectors of 131 chunks: more than
one 64-chunk workgroup of the scan, not a multiple of a wave or of a lane group."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gao_model as gm
import points_robust_model as prm
import zksaas_amd as zk
from zksaas_amd.api import ZK_G1, ZK_G2, unpack_points
from oracle.curve import g1, g2, GroupOps
from oracle.params import CURVES
from oracle.prng import rand_vec

from gpu_util import ctx, dec_jacobian, opp, up, up_parties

GROUPS = [("bn254", ZK_G1), ("bn254", ZK_G2), ("bls12_381", ZK_G1), ("bls12_381", ZK_G2), ("bls12_377", ZK_G1)]
CASES = [(c, g, l) for c, g in GROUPS for l in (1, 2, 4)] + [("bn254", ZK_G1, 8)]
IDS = ["%s_g%d_l%d" % c for c in CASES]
NCH = 131
SCAN_WG = 64          # chunks per workgroup of the scan (csrc/gao_points_impl.hpp GAO_PT_CHUNKS)


def _limbs(pp, group):
    """uint64 limbs of one affine point"""
    return pp.fq.nl * (4 if group == ZK_G2 else 2)


def _gen(pp, group):
    c = CURVES[pp.curve]
    flat = [c.g2[0][0], c.g2[0][1], c.g2[1][0], c.g2[1][1]] if group == ZK_G2 else list(c.g1)
    return np.ascontiguousarray(pp.fq.encode(flat).reshape(-1))


def _lift_d(pp, group, scalars_d, count):
    out = zk.DeviceBuffer(pp, max(1, count) * _limbs(pp, group) * 8)
    gen = _gen(pp, group)
    pp._check(pp.lib.zk_base_mul(pp.h, group, gen.ctypes.data, scalars_d.ptr, count, out.ptr, None))
    return out


def _lift(pp, group, scalars):
    """ints -> device affine points s G"""
    return _lift_d(pp, group, up(pp, scalars), len(scalars))


def _pts(pp, group, buf, count):
    return buf.to_numpy()[:count * _limbs(pp, group)].reshape(count, _limbs(pp, group))


def _columns(words, n):
    """chunk-major words -> one flat party-major list [n][len(words)]"""
    return [y[p] for p in range(n) for y in words]


def _consts(curve, l):
    o = opp(curve, l)
    return o.p, o.share.group_gen, o.secret.group_gen, o.curve.r_gen


@functools.lru_cache(maxsize=None)
def _model(curve, l):
    """{k: [(word, Decoded, secrets, repaired word)]} over the case list, decoded once per (curve, l)"""
    p, w, w2l, g = _consts(curve, l)
    by_k = {}
    for _, k, y in gm.case_list(l, p, w, 3):
        if k in (2 * l, 4 * l - 1):
            by_k.setdefault(k, []).append(_expect(curve, l, k, y))
    return by_k


def _expect(curve, l, k, y):
    p, w, w2l, g = _consts(curve, l)
    d, fixed = prm.repaired(y, k, w, p)
    sec = gm.secrets(d.message, l, g, w2l, p) if d.status != 2 else [0] * l
    return (list(y), d, sec, fixed)


def _want_summary(pick, n):
    return ([sum(1 for c in pick if c[1].status == s) for s in (0, 1, 2)] +
            [sum((c[1].errpos >> q) & 1 for c in pick) for q in range(n)])


def _check_unpack(pp, group, k, pick, tag):
    """one robust unpack and one repair of the words of `pick`, everything against the model"""
    n, l, nch = pp.n, pp.l, len(pick)
    sh = _lift(pp, group, _columns([c[0] for c in pick], n))
    r = pp.unpack_points_robust(group, sh, nch, k)
    assert list(r.status_host()) == [c[1].status for c in pick], tag
    assert list(r.errpos_host()) == [c[1].errpos for c in pick], tag
    assert r.summary == _want_summary(pick, n), tag
    want = _lift(pp, group, [v for c in pick for v in c[2]])
    assert np.array_equal(_pts(pp, group, r.out, nch * l), _pts(pp, group, want, nch * l)), tag
    rr = pp.repair_points(group, sh, nch, k)
    assert list(rr.status_host()) == [c[1].status for c in pick], tag
    assert list(rr.errpos_host()) == [c[1].errpos for c in pick], tag
    assert rr.summary == _want_summary(pick, n), tag
    fixed = _lift(pp, group, _columns([c[3] for c in pick], n))
    assert np.array_equal(_pts(pp, group, sh, n * nch), _pts(pp, group, fixed, n * nch)), tag
    return r


@pytest.mark.parametrize("curve,group,l", CASES, ids=IDS)
def test_case_vectors_equal_the_model(curve, group, l):
    pp = ctx(curve, l)
    by_k = _model(curve, l)
    assert sorted(by_k) == sorted({2 * l, 4 * l - 1})
    for k, cases in by_k.items():
        pick = [cases[c % len(cases)] for c in range(NCH)]
        if k == 2 * l and l >= 2:
            assert {c[1].status for c in pick} == {0, 1, 2}
        if k == 4 * l - 1:
            assert {c[1].status for c in pick} == {0, 2}          # detection only
        _check_unpack(pp, group, k, pick, (curve, group, l, k))


@pytest.mark.parametrize("curve,group,l", CASES, ids=IDS)
def test_clean_shares_equal_unpack_and_unpack2(curve, group, l):
    pp = ctx(curve, l)
    p = opp(curve, l).p
    n, w = pp.n, _limbs(pp, group)
    sh_fr = pp.pack(up(pp, rand_vec(140 + l, NCH * l, p)), NCH, seed=21)
    sh = _lift_d(pp, group, sh_fr, n * NCH)
    r = pp.unpack_points_robust(group, sh, NCH)
    assert not r.status_host().any() and not r.errpos_host().any()
    assert r.summary == [NCH, 0, 0] + [0] * n
    plain = unpack_points(pp, group, sh, NCH, two=False)
    assert np.array_equal(_pts(pp, group, r.out, NCH * l), _pts(pp, group, plain, NCH * l))
    # squared shares: degree <= 4l - 2, dimension 4l - 1
    rows = pp.download_fr(sh_fr, n * NCH)
    sq = _lift(pp, group, [int(v) * int(v) % p for v in rows])
    r2 = pp.unpack_points_robust(group, sq, NCH, 4 * l - 1)
    assert not r2.status_host().any()
    plain2 = unpack_points(pp, group, sq, NCH, two=True)
    assert np.array_equal(_pts(pp, group, r2.out, NCH * l), _pts(pp, group, plain2, NCH * l))


def test_six_chunks_against_the_oracle():
    """pss.rs:125-138 over group elements in the oracle's own curve arithmetic: chunks 0, 1, 63, 64, 65 and 130"""
    curve, l = "bn254", 2
    pp, o = ctx(curve, l), opp(curve, l)
    G = g1(CURVES[curve])
    ops = GroupOps(G)
    sh = _lift_d(pp, ZK_G1, pp.pack(up(pp, rand_vec(150, NCH * l, o.p)), NCH, seed=22), pp.n * NCH)
    r = pp.unpack_points_robust(ZK_G1, sh, NCH)
    nl = pp.fq.nl
    shares = _pts(pp, ZK_G1, sh, pp.n * NCH).reshape(pp.n, NCH, 2, nl)
    out = _pts(pp, ZK_G1, r.out, NCH * l).reshape(NCH, l, 2, nl)
    for c in (0, 1, 63, 64, 65, 130):
        word = [G.from_affine(tuple(pp.fq.decode(shares[q, c]))) for q in range(pp.n)]
        want = [G.to_affine(s) for s in o.unpack(word, ops)]
        assert [tuple(pp.fq.decode(out[c, i])) for i in range(l)] == [tuple(v) for v in want]


@pytest.mark.parametrize("curve,group,l", [("bn254", ZK_G1, 1), ("bn254", ZK_G1, 2), ("bn254", ZK_G2, 2),
                                           ("bls12_381", ZK_G2, 2), ("bn254", ZK_G1, 4)])
def test_one_lying_party_is_named_and_repaired(curve, group, l):
    pp = ctx(curve, l)
    p = opp(curve, l).p
    n = pp.n
    secrets = rand_vec(160 + l, NCH * l, p)
    honest_fr = pp.download_fr(pp.pack(up(pp, secrets), NCH, seed=23), n * NCH)
    honest = _pts(pp, group, _lift(pp, group, honest_fr), n * NCH).copy()
    want_out = _pts(pp, group, _lift(pp, group, secrets), NCH * l).copy()
    for bad in (0, n // 2 + 1, n - 1):
        cur = list(honest_fr)
        cur[bad * NCH:(bad + 1) * NCH] = rand_vec(170 + bad, NCH, p)
        sh = _lift(pp, group, cur)
        r = pp.unpack_points_robust(group, sh, NCH)
        assert set(r.status_host()) == {1} and set(r.errpos_host()) == {1 << bad}
        want = [0, NCH, 0] + [0] * n
        want[3 + bad] = NCH
        assert r.summary == want
        assert np.array_equal(_pts(pp, group, r.out, NCH * l), want_out)
        rr = pp.repair_points(group, sh, NCH)
        assert set(rr.status_host()) == {1} and set(rr.errpos_host()) == {1 << bad} and rr.summary == want
        assert np.array_equal(_pts(pp, group, sh, n * NCH), honest)          # the honest row's bytes, nothing else changed
        again = pp.repair_points(group, sh, NCH)
        assert not again.status_host().any() and again.summary == [NCH, 0, 0] + [0] * n
        assert np.array_equal(_pts(pp, group, sh, n * NCH), honest)


@pytest.mark.parametrize("group", [ZK_G1, ZK_G2])
def test_words_that_meet_the_special_cases_of_the_addition(group):
    curve, l = "bn254", 2
    pp = ctx(curve, l)
    p, w, _, _ = _consts(curve, l)
    n, k = pp.n, 2 * l
    code = gm.encode([11, 22, 33, 44], n, w, p)
    # a codeword with a root at w^5: (X - w^5)(7 + 9 X + 4 X^2)
    x5 = pow(w, 5, p)
    rooted = gm.encode(gm.poly_mul([(-x5) % p, 1], [7, 9, 4], p), n, w, p)
    assert rooted[5] == 0 and all(v for i, v in enumerate(rooted) if i != 5)
    words = [[0] * n,                                              # all shares the identity
             [5] * n,                                              # all shares one point: every addition of a row doubles
             [0 if q == 3 else v for q, v in enumerate(code)],     # a wrong share that is the identity
             [(-v) % p if q == 6 else v for q, v in enumerate(code)],      # a wrong share that is minus the true one
             [77 if q == 5 else v for q, v in enumerate(rooted)]]  # a true share that is the identity, with an error on it
    pick = [_expect(curve, l, k, y) for y in words]
    assert [(c[1].status, c[1].errpos) for c in pick] == [(0, 0), (0, 0), (1, 1 << 3), (1, 1 << 6), (1, 1 << 5)]
    _check_unpack(pp, group, k, pick, group)


def test_sizes_of_the_scan_and_of_the_dirty_list():
    curve, l = "bn254", 2
    pp = ctx(curve, l)
    p, w, _, _ = _consts(curve, l)
    n, k = pp.n, 2 * l
    groups_per_wg = 256 // n            # lane groups of one stage-2 workgroup

    def word(c, dirty):
        y = gm.encode([c + 1, c + 2, c + 3, c + 4], n, w, p)
        if dirty:
            y[c % n] = (y[c % n] + 9) % p
        return y

    r0 = pp.unpack_points_robust(ZK_G1, zk.DeviceBuffer(pp, 64), 0)
    assert r0.summary == [0] * (3 + n) and len(r0.status_host()) == 0
    shapes = [(1, set()), (1, {0}), (SCAN_WG - 1, {7}), (SCAN_WG, {0, SCAN_WG - 1}), (SCAN_WG + 1, {0, SCAN_WG}),
              (SCAN_WG + 1, set(range(SCAN_WG + 1)))]
    assert SCAN_WG + 1 > groups_per_wg
    for nch, dirty in shapes:
        pick = [_expect(curve, l, k, word(c, c in dirty)) for c in range(nch)]
        assert sum(c[1].status for c in pick) == len(dirty)
        _check_unpack(pp, ZK_G1, k, pick, (nch, sorted(dirty)[:3]))


def test_error_returns_leave_the_context_usable():
    pp = ctx("bn254", 2)
    p = opp("bn254", 2).p
    n, nch = pp.n, 7
    secrets = rand_vec(180, nch * 2, p)
    sh = _lift_d(pp, ZK_G1, pp.pack(up(pp, secrets), nch, seed=24), n * nch)
    st, out = zk.DeviceBuffer(pp, nch), zk.DeviceBuffer(pp, nch * 2 * _limbs(pp, ZK_G1) * 8)
    lib = pp.lib
    assert lib.zk_pss_unpack_points_robust(pp.h, ZK_G1, None, 0, 4, None, None, None, None, None) == 0
    assert lib.zk_pss_repair_points(pp.h, ZK_G1, None, 0, 4, None, None, None, None) == 0
    for bad_group in (0, 3):
        assert lib.zk_pss_unpack_points_robust(pp.h, bad_group, sh.ptr, nch, 4, out.ptr, st.ptr, None, None, None) == 4
        assert lib.zk_pss_repair_points(pp.h, bad_group, sh.ptr, nch, 4, st.ptr, None, None, None) == 4
    p377 = ctx("bls12_377", 2)          # no G2 on this curve
    assert p377.lib.zk_pss_unpack_points_robust(p377.h, ZK_G2, sh.ptr, nch, 4, None, st.ptr, None, None, None) == 4
    for bad_k in (0, -1, n, n + 5):
        assert lib.zk_pss_unpack_points_robust(pp.h, ZK_G1, sh.ptr, nch, bad_k, out.ptr, st.ptr, None, None, None) == 4
        assert lib.zk_pss_repair_points(pp.h, ZK_G1, sh.ptr, nch, bad_k, st.ptr, None, None, None) == 4
    for a, b in ((None, st.ptr), (sh.ptr, None)):
        assert lib.zk_pss_unpack_points_robust(pp.h, ZK_G1, a, nch, 4, out.ptr, b, None, None, None) == 4
        assert lib.zk_pss_repair_points(pp.h, ZK_G1, a, nch, 4, b, None, None, None) == 4
    # only shares and status are mandatory
    pp._check(lib.zk_pss_unpack_points_robust(pp.h, ZK_G1, sh.ptr, nch, 4, None, st.ptr, None, None, None))
    assert not st.to_numpy(np.uint8)[:nch].any()
    # the context is still usable
    r = pp.unpack_points_robust(ZK_G1, sh, nch)
    assert np.array_equal(_pts(pp, ZK_G1, r.out, nch * 2), _pts(pp, ZK_G1, _lift(pp, ZK_G1, secrets), nch * 2))


def _same_points(pp, group, a, b):
    """two [n][Jacobian] outputs hold the same n group elements.  zk_d_msm writes Jacobian coordinates, which are not
    canonical, and two calls of the unchanged zk_d_msm on one input differ in their bytes (the bucket sums are accumulated
    in whatever order the device takes them): each party's point is normalised to affine, and those are compared exactly."""
    is2 = group == ZK_G2
    G = (g2 if is2 else g1)(CURVES[pp.curve])
    return [G.to_affine(dec_jacobian(pp, r, is2)) for r in a] == [G.to_affine(dec_jacobian(pp, r, is2)) for r in b]


@pytest.mark.parametrize("group", [ZK_G1, ZK_G2])
def test_d_msm_checked(group):
    curve, l, ln = "bn254", 2, 300
    pp = ctx(curve, l)
    p = opp(curve, l).p
    n = pp.n
    # packed bases: det_pack of the discrete logs, lifted; packed scalars
    bases = _lift_d(pp, group, pp.det_pack(up(pp, rand_vec(190, ln * l, p)), ln), n * ln)
    scal_fr = pp.download_fr(pp.pack(up(pp, rand_vec(191, ln * l, p)), ln, seed=25), n * ln)
    scal = up(pp, scal_fr)
    mask = zk.MsmMask.sample(pp, group, _gen(pp, group), 26)
    for m in (zk.MsmMask.zero(), mask):
        out, status = pp.d_msm_checked(group, bases, scal, ln, m)
        assert status == 0
        assert _same_points(pp, group, out, zk.d_msm(pp, group, bases, scal, ln, m))
    # one party's scalar vector replaced
    bad = list(scal_fr)
    bad[3 * ln:4 * ln] = rand_vec(192, ln, p)
    bad_d = up(pp, bad)
    out, status = pp.d_msm_checked(group, bases, bad_d, ln, mask)
    assert status == 2
    assert _same_points(pp, group, out, zk.d_msm(pp, group, bases, bad_d, ln, mask))
    # one party's in-mask share replaced
    im = mask.in_mask.copy()
    assert not np.array_equal(im[1], im[2])
    im[1] = im[2]
    wrong = zk.MsmMask(im, mask.out_mask)
    out, status = pp.d_msm_checked(group, bases, scal, ln, wrong)
    assert status == 2
    assert _same_points(pp, group, out, zk.d_msm(pp, group, bases, scal, ln, wrong))
    with pytest.raises(zk.ZkError) as e:
        pp._check(pp.lib.zk_d_msm_checked(pp.h, group, bases.ptr, scal.ptr, ln, None, None, out.ctypes.data, None, None))
    assert e.value.code == 4
