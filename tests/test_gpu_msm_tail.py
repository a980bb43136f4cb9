"""The bucket tails of the Pippenger MSM (csrc/msm.hpp msm_heavy_kernel, msm_finalize_kernel, msm_reduce_a_kernel,
msm_reduce_b_kernel; csrc/quad.hpp qadd / qdbl / qaccum) at the shapes where their quads get none, one, two or many
points, through the C ABI.

The tails start every quad's sum from the first point it loads (a quad without one keeps the identity), stage B
enumerates the indices of a bit slice instead of filtering all of them, and qadd doubles equal points on a branch of its
own.  Every case multiplies chosen scalars against a few distinct bases repeated cyclically, so that the expected value
is one small oracle MSM over host-aggregated scalars whatever n is:

  * a 15-bit table (B = 2^14, 128 columns, 129 rows: two buckets per quad in stage A, the proof's shape) with digits that
    reach buckets 1, 2, B - 1 and B; 8- and 9-bit tables (LO != HI, groups shorter than the quads they get); table-free
    at 12 bits (many bucket sets); each single and as a batch of 3 (one-wave workgroups, another quads-per-group)
  * random scalars with 10 / 20 / 80 entries per bucket against 20 per accumulate lane (16 in G2): buckets inside one lane,
    over two, over three and more
  * a repeating-scalar vector (60 % ones, 25 % fives, 5 % r - 1) at 2^16 points: buckets of thousands of lanes, summed by
    one and by several virtual workgroups of msm_heavy_kernel and the finalize kernel's extra workgroups
  * ONE base with every bucket holding the same multiple of it (equal partial sums in finalize, in both stages and in
    every tree: the doubling branch) and the same with the sign alternating from bucket to bucket (partial sums that
    cancel: identity rows, identity leaves of the trees)
"""
import contextlib
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd.api import ZK_G1, ZK_G2, msm, msm_batch, msm_plan, msm_precompute, msm_table_info
from oracle.curve import g1, g2
from oracle.params import CURVES
from oracle.prng import rand_fp

import msm_digits as md
from gpu_util import enc_affine, dec_jacobian

NDIST = 40                       # distinct bases, repeated cyclically
GROUPS = [("bn254", "g1"), ("bn254", "g2"), ("bls12_381", "g1")]


@functools.lru_cache(maxsize=None)
def _distinct(curve, is2):
    cv = CURVES[curve]
    G = g2(cv) if is2 else g1(cv)
    gen = G.from_affine(G.gen)
    return G, G.batch_to_affine([G.mul(gen, rand_fp(80 + is2, i, cv.r)) for i in range(NDIST)])


@contextlib.contextmanager
def _own_context(curve, options):
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


def _check(curve, is2, c_req, table, vecs, points=None, cls=None):
    """msm (one vector) or msm_batch (several) of the canonical limb arrays `vecs` over points[cls[i]] (default: the NDIST
    distinct bases, cyclically, every 13th the identity) against the oracle's MSM over the aggregated scalars."""
    cv = CURVES[curve]
    r = cv.r
    G, distinct = _distinct(curve, is2)
    n = vecs[0].shape[0]
    if points is None:
        points, cls, live = distinct, np.arange(n) % NDIST, np.arange(n) % 13 != 7
    else:
        live = np.ones(n, dtype=bool)
    wants = [G.msm(points, md.aggregate(v, cls, len(points), live, r)) for v in vecs]
    geo = md.geometry(r, c_req, table) if c_req else None          # c_req None: the width the cost model picks
    group = ZK_G2 if is2 else ZK_G1
    opts = {("msm_table_c" if table else "msm_c") + ("_g2" if is2 else ""): c_req} if c_req else {}
    with _own_context(curve, opts) as (pp, dev):
        rows = enc_affine(pp, points, is2)[cls]
        rows[~live] = 0
        bases = dev(rows)
        scs = [dev(md.montgomery_limbs(v, r)) for v in vecs]
        if table:
            msm_precompute(pp, group, bases, n)
            assert msm_table_info(pp, group, bases) == {"window_bits": geo.c, "windows": geo.nwin}
        elif geo:
            plan = msm_plan(pp, group, n)
            assert (plan["window_bits"], plan["windows"]) == (geo.c, geo.nwin)
        out = [msm(pp, group, bases, scs[0], n)] if len(vecs) == 1 else msm_batch(pp, group, bases, scs, n)
        gots = [dec_jacobian(pp, o, is2) for o in out]
    for k, (got, want) in enumerate(zip(gots, wants)):
        assert G.is_identity(got) == G.is_identity(want), "scalar vector %d" % k
        assert G.eq(got, want), "scalar vector %d" % k
    return wants


# ------------------------------------------------------------------------------------------ engineered digits
@functools.lru_cache(maxsize=None)
def _engineered(curve, c_req, table):
    """Engineered scalars (tests/msm_digits.py) that reach magnitudes B, B - 1, 1 and 2 in every freely chosen window, an
    even stride over the rest up to 4096, and the edge scalars; the same length of edge scalars repeated; +half in
    every window of every scalar."""
    r = CURVES[curve].r
    geo = md.geometry(r, c_req, table)
    nl = (geo.bits + 63) // 64
    idx = md.table_indices(geo, 4096)
    digs = md.engineered_digit_array(r, geo, idx)
    for w in range(md.free_windows(r, geo)):
        h = md.half(geo, w)
        live = (np.arange(digs.shape[0]) % 13 != 7)
        mag = np.abs(digs[live, w])
        for k in {h, h - 1, 1, min(2, h)} - {0}:
            assert (mag == k).any(), (c_req, w, k)
    edges = md.edge_scalars(r, geo)
    el = md.ints_to_limbs(edges, nl)
    limbs = np.concatenate([md.digits_to_limbs(digs, geo, nl), el])
    n = limbs.shape[0]
    return limbs, el[np.arange(n) % len(edges)], np.repeat(md.ints_to_limbs([md.half_digit_scalar(r, geo)], nl), n, axis=0)


SHAPES = [(15, True), (8, True), (9, True), (12, False)]


@pytest.mark.parametrize("c_req,table", SHAPES, ids=["table15", "table8", "table9", "free12"])
@pytest.mark.parametrize("curve,grp", GROUPS)
def test_engineered_digits_single(curve, grp, c_req, table):
    """Row HI (bucket B), row slice hb and every column slice are non-empty; at 8 and 9 bits rows and columns differ in
    number and stage A has more quads than a group has buckets."""
    _check(curve, grp == "g2", c_req, table, _engineered(curve, c_req, table)[:1])


@pytest.mark.parametrize("c_req,table", SHAPES, ids=["table15", "table8", "table9", "free12"])
@pytest.mark.parametrize("curve,grp", GROUPS)
def test_engineered_digits_batch_of_3(curve, grp, c_req, table):
    """One-wave workgroups: 16 quads per workgroup, several buckets per quad in stage A; the third vector puts every
    entry of a window into one bucket (msm_heavy_kernel)."""
    _check(curve, grp == "g2", c_req, table, list(_engineered(curve, c_req, table)))


# ------------------------------------------------------------------------------------------ lanes per bucket
def _random_limbs(seed, n, r):
    nl = (r.bit_length() + 63) // 64
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 62, size=(n, nl), dtype=np.uint64)
    a[:, nl - 1] &= np.uint64((1 << 58) - 1)               # below r on every curve here
    return a


@pytest.mark.parametrize("per_bucket", (10, 20, 80))
@pytest.mark.parametrize("curve,grp", GROUPS)
def test_buckets_inside_one_lane_over_two_and_over_more(curve, grp, per_bucket):
    """Table-free at 8 bits: 128 buckets per window, n / 128 entries per bucket against accumulate ranges of 20 entries (16
    in G2): most buckets inside one range, most over two, every bucket over four to six (tail + several heads per quad in
    the finalize kernel)."""
    r = CURVES[curve].r
    _check(curve, grp == "g2", 8, False, [_random_limbs(per_bucket, 128 * per_bucket, r)])


# ------------------------------------------------------------------------------------------ heavy buckets
@pytest.mark.parametrize("curve,grp", [("bn254", "g1"), ("bls12_381", "g1")])
def test_repeating_scalars_heavy_buckets_with_one_and_several_workgroups(curve, grp):
    """2^16 points, 60 % ones, 25 % fives, 5 % r - 1, the rest random (tools/skew_msm.py): the buckets of 1 and 5 span
    about 2000 and 800 accumulate lanes (several virtual workgroups each: chunk sums in hpart[], summed by the finalize
    kernel's extra workgroups), the buckets of r - 1 between 16 and 256 (one virtual workgroup)."""
    r = CURVES[curve].r
    n = 1 << 16
    limbs = _random_limbs(5, n, r)
    nl = limbs.shape[1]
    sel = np.random.default_rng(6).random(n)
    for lo, hi, val in ((0.0, 0.6, 1), (0.6, 0.85, 5), (0.85, 0.9, r - 1)):
        limbs[(sel >= lo) & (sel < hi)] = md.ints_to_limbs([val], nl)[0]
    _check(curve, grp == "g2", None, False, [limbs])


# ------------------------------------------------------------------------------------------ equal and opposite partial sums
def _flat(curve, is2, c_req, kmax, m, alternate):
    """n = kmax * m points, scalar k = 1..kmax m times each (one non-zero digit, in window 0: bucket k gets m entries), all
    on ONE base P -- or on P for even k and -P for odd k.  Every bucket then holds m P (or -m P): the sums of equal
    buckets, rows, columns and tree leaves are doublings; neighbouring buckets of opposite sign cancel."""
    cv = CURVES[curve]
    G, distinct = _distinct(curve, is2)
    P = distinct[0]
    nP = G.to_affine(G.neg(G.from_affine(P)))
    geo = md.geometry(cv.r, c_req, True)
    assert kmax <= geo.B and md.recode(kmax, geo)[0] == kmax and not any(md.recode(kmax, geo)[1:])
    k = np.tile(np.arange(1, kmax + 1, dtype=np.uint64), m)
    limbs = np.zeros((k.size, (geo.bits + 63) // 64), dtype=np.uint64)
    limbs[:, 0] = k
    cls = (k & np.uint64(1)).astype(np.int64) if alternate else np.zeros(k.size, dtype=np.int64)
    return limbs, [P, nP], cls


# (table bits, buckets used, entries per bucket): 8 bits: all 128 buckets, rows of 16; 15 bits: the first 16 of 129 rows,
# two buckets per quad in stage A.  24 / 48 entries per bucket against ranges of 20 (16): every bucket straddles lanes, and
# where a bucket begins on a lane boundary its tail and heads are equal partial sums in the finalize kernel.
FLAT = [(8, 128, 48), (15, 2048, 24)]


@pytest.mark.parametrize("alternate", (False, True), ids=["equal", "opposite"])
@pytest.mark.parametrize("c_req,kmax,m", FLAT, ids=["table8", "table15"])
@pytest.mark.parametrize("curve,grp", GROUPS)
def test_equal_and_opposite_partial_sums(curve, grp, c_req, kmax, m, alternate):
    is2 = grp == "g2"
    limbs, pts, cls = _flat(curve, is2, c_req, kmax, m, alternate)
    _check(curve, is2, c_req, True, [limbs], pts, cls)


@pytest.mark.parametrize("alternate", (False, True), ids=["equal", "opposite"])
@pytest.mark.parametrize("grp", ("g1", "g2"))
def test_equal_and_opposite_partial_sums_batch_of_3(grp, alternate):
    """One-wave workgroups.  The third vector is the first one backwards: bucket k swaps with bucket 129 - k."""
    is2 = grp == "g2"
    limbs, pts, cls = _flat("bn254", is2, 8, 128, 48, alternate)
    _check("bn254", is2, 8, True, [limbs, limbs.copy(), limbs[::-1].copy()], pts, cls)


def test_everything_cancels_to_the_identity():
    """P and -P on the SAME scalars: every bucket is the identity when the accumulate kernel is done, or cancels in the
    finalize kernel; both stages and the host fold see identities only and the result is the identity."""
    limbs, pts, _ = _flat("bn254", False, 8, 128, 48, False)
    cls = (np.arange(limbs.shape[0]) // 128 % 2).astype(np.int64)         # whole runs of 1..128 alternate in sign
    want = _check("bn254", False, 8, True, [limbs], pts, cls)[0]
    assert _distinct("bn254", False)[0].is_identity(want)
