"""The Pippenger MSM at every window width, with scalars built digit by digit (tests/msm_digits.py), through the C ABI.

Random scalars reach the largest bucket of a window (k = B = 2^(c-1): the extra row of reduce stage A, row slice hb of
stage B, sl[hb] in the host fold) with probability 2^-c per (point, window), never produce a +half digit in every
window at once, and rarely a long carry chain.  Here every case multiplies 2B engineered scalars -- every digit of
(-half, +half] in every freely chosen window, checked on the host before the launch -- plus the edge scalars (carry
chains of every length, +half and half + 1 alone in every window) against a few dozen distinct bases repeated
cyclically with identity bases sprinkled in, so that the expected value is one small oracle MSM over host-aggregated
scalars whatever n is.  Per case: result == oracle, the plan / table geometry equals the one restated in Python, and
zk_msm_stats counts exactly the non-zero digits on non-identity bases (the two digit walkers of the sort paths must
agree with the Python recoding to the entry) and n x windows offered pairs.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd.api import ZK_G1, ZK_G2, msm, msm_batch, msm_plan, msm_precompute, msm_table_info
from oracle import dist as od
from oracle.curve import g1, g2, GroupOps
from oracle.params import CURVES
from oracle.prng import rand_fp

import msm_digits as md
from gpu_util import opp, enc_affine, dec_jacobian

NDIST = 48                       # distinct bases, repeated cyclically
ATOMICS, LDS = 1 << 40, 0        # msm_bigsort_min: the global-atomics sort / the two-level LDS sort at every size


def _live(n):
    """identity bases: one early, then every eleventh (a CRS is full of them)"""
    i = np.arange(n)
    return (i != 5) & (i % 11 != 3)


@functools.lru_cache(maxsize=None)
def _distinct(curve, is2):
    cv = CURVES[curve]
    G = g2(cv) if is2 else g1(cv)
    gen = G.from_affine(G.gen)
    return G, G.batch_to_affine([G.mul(gen, rand_fp(64 + is2, i, cv.r)) for i in range(NDIST)])


_ROWS = {}


def _base_rows(pp, curve, is2, n):
    """[n][affine limbs]: distinct[i mod 48], zeros (the identity) where not _live"""
    if (curve, is2) not in _ROWS:
        _ROWS[curve, is2] = enc_affine(pp, _distinct(curve, is2)[1], is2)
    rows = _ROWS[curve, is2][np.arange(n) % NDIST]
    rows[~_live(n)] = 0
    return rows


@functools.lru_cache(maxsize=2)
def _scalars(curve, c_req, table):
    """(geometry, canonical limbs [n][nl], non-zero digits per scalar [n]) of the engineered + edge vector; asserts that
    the scalars on non-identity bases reach the largest bucket, the one below it and buckets 1 and 2 of every freely chosen
    window."""
    r = CURVES[curve].r
    geo = md.geometry(r, c_req, table)
    nl = (geo.bits + 63) // 64
    idx = md.table_indices(geo) if table else None          # all 2B unless a table above 16 bits: 2^16 chosen ones
    digs = md.engineered_digit_array(r, geo, idx)
    edges = md.edge_scalars(r, geo)
    limbs = np.concatenate([md.digits_to_limbs(digs, geo, nl), md.ints_to_limbs(edges, nl)])
    nz = np.concatenate([(digs != 0).sum(axis=1), np.array([md.nonzero_digits(s, geo) for s in edges])])
    live = _live(limbs.shape[0])[: digs.shape[0]]
    for w in range(md.free_windows(r, geo)):
        h = md.half(geo, w)
        mag = np.abs(digs[live, w])
        for k in {h, h - 1, 1, min(2, h)} - {0}:            # buckets B (or B/2 in a narrow window), the one below, 1 and 2
            assert (mag == k).any(), (c_req, w, k)
    return geo, limbs, nz


_WANT = {}


def _expected(curve, is2, key, limbs):
    """sum_i s_i P_(i mod 48) over the non-identity bases: the oracle's MSM over the 48 aggregated scalars"""
    if (curve, is2, key) not in _WANT:
        G, distinct = _distinct(curve, is2)
        n = limbs.shape[0]
        agg = md.aggregate(limbs, np.arange(n) % NDIST, NDIST, _live(n), CURVES[curve].r)
        assert any(agg)
        want = G.msm(distinct, agg)
        assert not G.is_identity(want)
        _WANT[curve, is2, key] = want
    return _WANT[curve, is2, key]


def _stats(pp):
    st = (C.c_uint64 * 4)()
    pp._check(pp.lib.zk_msm_stats(pp.h, st))
    return list(st)


@contextlib.contextmanager
def _own_context(curve, options):
    """A context of the case's own (options must not leak); its device buffers go before it (tables are found by
    address: zk_free drops them)."""
    pp = zk.PackedSharingParams(curve, 2)
    bufs = []

    def dev(arr):
        bufs.append(zk.DeviceBuffer.from_numpy(pp, arr))
        return bufs[-1]

    try:
        for name, value in options.items():
            pp.set_option(name, value)
        yield pp, dev
    finally:
        for b in bufs:
            b.free()
        pp.close()


def _options(is2, c_req, table, bigsort):
    opt = {("msm_table_c" if table else "msm_c") + ("_g2" if is2 else ""): c_req}
    if bigsort is not None:
        opt["msm_bigsort_min"] = bigsort
    return opt


def _check_geometry(pp, group, bases, n, geo, table):
    if table:
        msm_precompute(pp, group, bases, n)
        assert msm_table_info(pp, group, bases) == {"window_bits": geo.c, "windows": geo.nwin}
    else:
        plan = msm_plan(pp, group, n)
        assert (plan["window_bits"], plan["windows"]) == (geo.c, geo.nwin)
        assert geo.c <= geo.c_req


def _run(curve, group, c_req, bigsort=None, table=False):
    is2 = group == ZK_G2
    r = CURVES[curve].r
    G = _distinct(curve, is2)[0]
    geo, limbs, nz = _scalars(curve, c_req, table)
    n = limbs.shape[0]
    want = _expected(curve, is2, (c_req, table), limbs)
    with _own_context(curve, _options(is2, c_req, table, bigsort)) as (pp, dev):
        bases = dev(_base_rows(pp, curve, is2, n))
        sc = dev(md.montgomery_limbs(limbs, r))
        _check_geometry(pp, group, bases, n, geo, table)
        st0 = _stats(pp)
        got = dec_jacobian(pp, msm(pp, group, bases, sc, n), is2)
        st1 = _stats(pp)
    assert G.eq(got, want)
    assert st1[is2] - st0[is2] == int(nz[_live(n)].sum()), "mixed additions != non-zero digits on non-identity bases"
    assert st1[2 + is2] - st0[2 + is2] == n * geo.nwin
    assert st1[1 - is2] == st0[1 - is2] and st1[3 - is2] == st0[3 - is2]


def _ids(cases):
    return [pytest.param(*c, id="-".join(str(x) for x in c)) for c in cases]


@pytest.mark.parametrize("c_req,path", _ids([(c, p) for c in range(2, 13) for p in ("lds", "atomics")] +
                                             [(c, "default") for c in range(13, 21)]))
def test_bn254_g1_every_width(c_req, path):
    """Every accepted msm_c.  c_req = 20: 2^20 + edge scalars, 13 x 2^19 buckets."""
    _run("bn254", ZK_G1, c_req, {"lds": LDS, "atomics": ATOMICS, "default": None}[path])


@pytest.mark.parametrize("c_req", (2, 3, 7, 8, 12, 13, 16))
@pytest.mark.parametrize("curve,grp", [("bn254", "g2"), ("bls12_381", "g1"), ("bls12_381", "g2"), ("bls12_377", "g1")])
def test_other_groups_forced_widths(curve, grp, c_req):
    """Odd and even c, wide == nwin and wide < nwin, lo_bits 1..8, both sides of the 64-quad tree of reduce stage A; the
    quad-split extension-field kernels and the 12-limb fields."""
    _run(curve, ZK_G2 if grp == "g2" else ZK_G1, c_req)


@pytest.mark.parametrize("c_req", (19, 20))
def test_bls12_381_g1_widest(c_req):
    _run("bls12_381", ZK_G1, c_req)


@pytest.mark.parametrize("curve,grp,c_req", _ids([("bn254", "g1", c) for c in (8, 9, 12, 15, 16, 17, 20, 22)] +
                                                  [("bn254", "g2", c) for c in (8, 13, 16)] +
                                                  [("bls12_381", "g1", c) for c in (8, 13, 16)]))
def test_fixed_base_tables(curve, grp, c_req):
    """All windows share ONE bucket set: the narrow windows reach only its lower half and the host fold sees a single
    c-bit window.  Above 16 bits: 2^16 of the 2B engineered scalars (msm_digits.table_indices) + the edge scalars."""
    _run(curve, ZK_G2 if grp == "g2" else ZK_G1, c_req, table=True)


def test_table_width_below_8_is_refused():
    """msm_table_c accepts 8..22: the batch matrix below has no (3 bits, table) case."""
    with _own_context("bn254", {}) as (pp, _):
        for name in ("msm_table_c", "msm_table_c_g2"):
            for bad in (3, 7, 23):
                with pytest.raises(zk.ZkError) as e:
                    pp.set_option(name, bad)
                assert e.value.code == 4


@pytest.mark.parametrize("grp,c_req,table", _ids([(g, c, t) for g in ("g1", "g2") for t in ("tablefree", "table")
                                                  for c in (3, 8, 13) if (c, t) != (3, "table")]))
def test_batches(grp, c_req, table):
    """zk_msm_batch (one-wave workgroups in the reduce kernels, bucket sets per scalar vector): the engineered vector, the
    edge scalars repeated to the same length, and +half in every window of every scalar (one heavy bucket per window)."""
    curve, is2, table = "bn254", grp == "g2", table == "table"
    group = ZK_G2 if is2 else ZK_G1
    r = CURVES[curve].r
    G = _distinct(curve, is2)[0]
    geo, limbs, nz = _scalars(curve, c_req, table)
    n, nl = limbs.shape
    edges = md.edge_scalars(r, geo)
    el, enz = md.ints_to_limbs(edges, nl), np.array([md.nonzero_digits(s, geo) for s in edges])
    rep = np.arange(n) % len(edges)
    hs = md.half_digit_scalar(r, geo)
    vecs = [(limbs, nz), (el[rep], enz[rep]),
            (np.repeat(md.ints_to_limbs([hs], nl), n, axis=0), np.full(n, md.nonzero_digits(hs, geo)))]
    wants = [_expected(curve, is2, (c_req, table, "batch", k), v[0]) for k, v in enumerate(vecs)]
    with _own_context(curve, _options(is2, c_req, table, None)) as (pp, dev):
        bases = dev(_base_rows(pp, curve, is2, n))
        scs = [dev(md.montgomery_limbs(v[0], r)) for v in vecs]
        _check_geometry(pp, group, bases, n, geo, table)
        st0 = _stats(pp)
        out = msm_batch(pp, group, bases, scs, n)
        st1 = _stats(pp)
        gots = [dec_jacobian(pp, o, is2) for o in out]
    for k, (got, want) in enumerate(zip(gots, wants)):
        assert G.eq(got, want), "scalar vector %d" % k
    live = _live(n)
    assert st1[is2] - st0[is2] == sum(int(v[1][live].sum()) for v in vecs)
    assert st1[2 + is2] - st0[2 + is2] == len(vecs) * n * geo.nwin


@pytest.mark.parametrize("path", ("lds", "atomics"))
@pytest.mark.parametrize("c_req", (8, 13))
def test_d_msm_digits_chosen_before_the_party_coefficients(c_req, path):
    """zk_d_msm multiplies every party's scalars by its unpack2 coefficient inside the sort kernels (csrc/msm.hpp
    d_msm_range_t: coef_p = sum_k unpack2(e_p)[k]), so the digits are chosen BEFORE that product: the scalars handed in
    are the engineered ones divided by coef_p mod r.  Expected shares: oracle.dist.d_msm."""
    curve, l = "bn254", 2
    cv = CURVES[curve]
    r = cv.r
    G, distinct = _distinct(curve, False)
    o = opp(curve, l)
    coef = [sum(o.unpack2([int(k == p) for k in range(o.n)])) % r for p in range(o.n)]
    assert all(coef)
    geo, limbs, _ = _scalars(curve, c_req, False)
    e = md.limbs_to_ints(limbs)
    edges = md.edge_scalars(r, geo)
    e += [edges[k % len(edges)] for k in range(-len(e) % o.n)]           # a whole number of points per party
    ln = len(e) // o.n
    y = [s * pow(coef[i // ln], -1, r) % r for i, s in enumerate(e)]
    assert all(v * coef[i // ln] % r == e[i] for i, v in enumerate(y))
    n = len(e)
    live = _live(n)
    aggs = []
    for p in range(o.n):
        agg = [0] * NDIST
        for i in range(p * ln, (p + 1) * ln):
            if live[i]:
                agg[i % NDIST] = (agg[i % NDIST] + y[i]) % r
        aggs.append(agg)
    assert any(any(a) for a in aggs)
    want = od.d_msm([distinct] * o.n, aggs, [od.MsmMask.zero(G)] * o.n, o, G, GroupOps(G))
    assert not G.is_identity(want[0])
    opts = _options(False, c_req, False, LDS if path == "lds" else ATOMICS)
    with _own_context(curve, opts) as (pp, dev):
        assert pp.n == o.n
        bases = dev(_base_rows(pp, curve, False, n))
        sc = dev(md.montgomery_limbs(md.ints_to_limbs(y, limbs.shape[1]), r))
        plan = msm_plan(pp, ZK_G1, n)
        assert (plan["window_bits"], plan["windows"]) == (geo.c, geo.nwin)
        st0 = _stats(pp)
        out = zk.d_msm(pp, ZK_G1, bases, sc, ln)
        st1 = _stats(pp)
        gots = [dec_jacobian(pp, out[p]) for p in range(o.n)]
    for p in range(o.n):
        assert G.eq(gots[p], want[p]), "party %d" % p
    assert st1[0] - st0[0] == sum(md.nonzero_digits(s, geo) for i, s in enumerate(e) if live[i])
    assert st1[2] - st0[2] == n * geo.nwin
