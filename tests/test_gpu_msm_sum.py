"""zk_msm_sum: up to three MSMs of one group end in ONE shared bucket set (csrc/msm.hpp "SHARED BUCKET SET": donor launches
stop behind msm_finalize_kernel, the last launch's finalize kernel adds their buckets to its own through qadd) -- the path
that ends r*H + W + U of a full proof.  Every case compares, as a group element, with the sum of separate zk_msm results and
with ONE small oracle MSM over host-aggregated scalars (the vectors repeat a few distinct bases cyclically), and asserts
whether the launches shared a bucket set or fell back to reductions of their own.

The vectors are registered with the default table (15 bits: one set of 2^14 buckets, the proof's geometry), so the bucket
count does not depend on the length and the shapes stay small:

  * 1 point per vector and 3 vectors of 64 points: every non-empty bucket lies inside one accumulate lane's range (written
    by the accumulate kernel, untouched by the finalize kernel of a lone MSM) and almost every bucket is empty
  * 8 192 points whose scalars take 4 distinct values: 17 x 4 buckets that straddle hundreds of lanes (msm_heavy_kernel, with
    one and with several virtual workgroups: the buckets the finalize kernel's extra workgroups sum and merge)
  * the same registered vector twice with the same scalars: every bucket doubles (qadd's equal-points branch)
  * scalars x and r - x on the same vector: every bucket cancels; all-zero scalars: every donated bucket is empty
  * a vector with a table and one without, two tables of different width, table-free vectors: the fallback path
  * two calls in flight from two host threads on two streams: the donors' workspace slots
"""
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd.api import ZK_G1, ZK_G2, msm, msm_sum, msm_precompute, msm_stats, msm_table_info
from oracle.curve import g1, g2
from oracle.params import BN254
from oracle.prng import rand_fp

import msm_digits as md
from gpu_util import enc_affine, dec_jacobian

R = BN254.r
NL = 4
NDIST = 24


@functools.lru_cache(maxsize=None)
def _distinct(is2):
    G = g2(BN254) if is2 else g1(BN254)
    gen = G.from_affine(G.gen)
    return G, G.batch_to_affine([G.mul(gen, rand_fp(90 + is2, i, R)) for i in range(NDIST)])


def _random(seed, n):
    a = np.random.default_rng(seed).integers(0, 1 << 62, size=(n, NL), dtype=np.uint64)
    a[:, NL - 1] &= np.uint64((1 << 58) - 1)
    return a


class _Ctx:
    """A context of its own (tables and table options belong to it) with vectors that repeat the distinct bases cyclically
    from a per-vector offset, every 13th base the identity."""

    def __init__(self, is2=False, options=None):
        self.is2, self.group = is2, ZK_G2 if is2 else ZK_G1
        self.G, self.pts = _distinct(is2)
        self.pp = zk.PackedSharingParams("bn254", 2)
        for k, v in (options or {}).items():
            self.pp.set_option(k, v)
        self.bufs = []

    def dev(self, arr):
        self.bufs.append(zk.DeviceBuffer.from_numpy(self.pp, np.ascontiguousarray(arr)))
        return self.bufs[-1]

    def vector(self, n, shift, table=True):
        cls = (np.arange(n) + shift) % NDIST
        live = np.arange(n) % 13 != 7 if n > 1 else np.ones(n, dtype=bool)
        rows = enc_affine(self.pp, self.pts, self.is2)[cls]
        rows[~live] = 0
        buf = self.dev(rows)
        if table:
            msm_precompute(self.pp, self.group, buf, n)
            assert msm_table_info(self.pp, self.group, buf)["window_bits"] == 15
        return buf, cls, live

    def close(self):
        for b in self.bufs:
            b.free()
        self.pp.close()

    def check(self, items, shared):
        """items: [(vector, canonical scalar limbs)]: zk_msm_sum == sum of zk_msm == oracle; returns the oracle's point"""
        pp, G = self.pp, self.G
        agg = [0] * NDIST
        triples, singles = [], G.identity
        for (buf, cls, live), limbs in items:
            n = limbs.shape[0]
            for j, v in enumerate(md.aggregate(limbs, cls, NDIST, live, R)):
                agg[j] = (agg[j] + v) % R
            sc = self.dev(md.montgomery_limbs(limbs, R))
            triples.append((buf, sc, n))
            singles = G.add(singles, dec_jacobian(pp, msm(pp, self.group, buf, sc, n), self.is2))
        want = G.msm(self.pts, agg)
        before = msm_stats(pp)
        out, nshared = msm_sum(pp, self.group, triples, with_shared=True)
        after = msm_stats(pp)
        got = dec_jacobian(pp, out, self.is2)
        assert nshared == shared
        assert G.is_identity(got) == G.is_identity(want) and G.eq(got, want)
        assert G.eq(got, singles)
        return want, before, after


@pytest.fixture
def c1():
    c = _Ctx(False)
    yield c
    c.close()


@pytest.mark.parametrize("n,k", [(1, 3), (64, 3), (64, 2), (64, 1)])
def test_buckets_inside_one_lane_merge(c1, n, k):
    vecs = [c1.vector(n, 5 * i) for i in range(k)]
    c1.check([(v, _random(10 + i, n)) for i, v in enumerate(vecs)], k - 1)


def test_g2_merges_too():
    c = _Ctx(True)
    try:
        vecs = [c.vector(64, 3 * i) for i in range(3)]
        c.check([(v, _random(20 + i, 64)) for i, v in enumerate(vecs)], 2)
    finally:
        c.close()


def test_heavy_buckets_merge(c1):
    """4 distinct scalar values over 8 192 points: a value's bucket in each of the 17 windows holds ~2 000 entries = ~100
    accumulate lanes (one virtual workgroup of msm_heavy_kernel); with 60 % of the points on one value its buckets span
    more than 256 lanes (several virtual workgroups, summed AND merged by the finalize kernel's extra workgroups)."""
    n = 8192
    vals = md.ints_to_limbs([rand_fp(30, i, R) for i in range(4)], NL)
    even = vals[np.arange(n) % 4]
    skew = vals[np.where(np.random.default_rng(31).random(n) < 0.8, 0, np.arange(n) % 4)]
    vecs = [c1.vector(n, 7 * i) for i in range(3)]
    c1.check([(vecs[0], even), (vecs[1], skew), (vecs[2], skew[::-1].copy())], 2)
    c1.check([(vecs[0], _random(32, n)), (vecs[1], _random(33, n)), (vecs[2], skew)], 2)


def test_same_vector_twice_doubles_every_bucket(c1):
    n = 64
    v = c1.vector(n, 0)
    limbs = _random(40, n)
    want, before, after = c1.check([(v, limbs), (v, limbs)], 1)
    one = c1.G.msm(c1.pts, md.aggregate(limbs, v[1], NDIST, v[2], R))
    assert c1.G.eq(want, c1.G.add(one, one))


def test_opposite_scalars_cancel_every_bucket(c1):
    n = 64
    v = c1.vector(n, 0)
    x = _random(41, n)
    neg = md.ints_to_limbs([(R - s) % R for s in md.limbs_to_ints(x)], NL)
    want, _, _ = c1.check([(v, x), (v, neg)], 1)
    assert c1.G.is_identity(want)


def test_all_zero_scalars_donate_empty_buckets(c1):
    n = 64
    vecs = [c1.vector(n, 4 * i) for i in range(3)]
    zero = np.zeros((n, NL), dtype=np.uint64)
    c1.check([(vecs[0], zero), (vecs[1], _random(42, n)), (vecs[2], _random(43, n))], 2)
    c1.check([(vecs[0], _random(44, n)), (vecs[1], zero), (vecs[2], zero)], 2)


def test_stats_count_what_separate_msms_count(c1):
    n = 64
    vecs = [c1.vector(n, 4 * i) for i in range(3)]
    sc = [c1.dev(md.montgomery_limbs(_random(50 + i, n), R)) for i in range(3)]
    pp = c1.pp
    s0 = msm_stats(pp)
    for v, s in zip(vecs, sc):
        msm(pp, ZK_G1, v[0], s, n)
    s1 = msm_stats(pp)
    msm_sum(pp, ZK_G1, [(v[0], s, n) for v, s in zip(vecs, sc)])
    s2 = msm_stats(pp)
    assert [b - a for a, b in zip(s0, s1)] == [b - a for a, b in zip(s1, s2)]


def test_different_geometries_fall_back(c1):
    """a table on one vector only (one bucket set against one per window), then three table-free vectors of one length (the
    same windows: shared) and of very different lengths (other window bits)."""
    n = 64
    tab, free = c1.vector(n, 0), c1.vector(n, 3, table=False)
    c1.check([(tab, _random(60, n)), (free, _random(61, n))], 0)
    c1.check([(free, _random(62, n)), (tab, _random(63, n))], 0)
    free2 = c1.vector(n, 9, table=False)
    c1.check([(free, _random(64, n)), (free2, _random(65, n)), (free, _random(66, n))], 2)
    big = c1.vector(4096, 1, table=False)
    c1.check([(free, _random(67, n)), (big, _random(68, 4096))], 0)
    # mixed: the middle vector matches the last one, the first does not
    tab2 = c1.vector(n, 11)
    c1.check([(free, _random(69, n)), (tab, _random(70, n)), (tab2, _random(71, n))], 1)


def test_tables_of_different_width_fall_back():
    c = _Ctx(False)
    try:
        n = 64
        a = c.vector(n, 0)
        c.pp.set_option("msm_table_c", 12)
        rows = enc_affine(c.pp, c.pts, False)[(np.arange(n) + 2) % NDIST]
        buf = c.dev(rows)
        msm_precompute(c.pp, ZK_G1, buf, n)
        assert msm_table_info(c.pp, ZK_G1, buf)["window_bits"] != 15
        b = (buf, (np.arange(n) + 2) % NDIST, np.ones(n, dtype=bool))
        c.check([(a, _random(80, n)), (b, _random(81, n))], 0)
    finally:
        c.close()


def test_two_calls_in_flight_from_two_streams(c1):
    """Two host threads, a stream each, the same context: the calls take turns on the standalone slots (the donors' slots are
    busy until the absorbing launch has been joined) and both results are right, several times over."""
    import torch
    n = 2048
    vecs = [c1.vector(n, 5 * i) for i in range(3)]
    pp, G = c1.pp, c1.G
    jobs = []
    for t in range(2):
        limbs = [_random(100 + 10 * t + i, n) for i in range(3)]
        agg = [0] * NDIST
        for v, l_ in zip(vecs, limbs):
            for j, a in enumerate(md.aggregate(l_, v[1], NDIST, v[2], R)):
                agg[j] = (agg[j] + a) % R
        jobs.append(([(v[0], c1.dev(md.montgomery_limbs(l_, R)), n) for v, l_ in zip(vecs, limbs)], G.msm(c1.pts, agg)))
    streams = [torch.cuda.Stream() for _ in range(2)]
    results = [[], []]

    def run(t):
        for _ in range(4):
            results[t].append(msm_sum(pp, ZK_G1, jobs[t][0], stream=streams[t].cuda_stream, with_shared=True))

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for t in range(2):
        assert len(results[t]) == 4
        for out, nshared in results[t]:
            assert nshared == 2
            assert G.eq(dec_jacobian(pp, out), jobs[t][1])
