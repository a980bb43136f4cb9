"""GPU tests (through the C ABI) for zk_pss_repair_batch_parties: zk_pss_repair_parties of several COMPACT share matrices
[nparties][nchunks] of ONE party list, item i at shares_d + i * item_stride, with the launches of zk_pss_repair_batch (one scan
with the item on grid.y, one decoder launch over ONE list of dirty (item, chunk) entries) and the two tables of the list put
into working memory once per call.
  yardstick      nitems calls of zk_pss_repair_parties on copies of the same matrices: shares, status, errpos and summary are
                 equal byte for byte, per item; the pad between two items keeps its bytes
  contents       per item: a listed liar in every chunk (named and repaired where the list leaves a cap >= 1), the liar absent
                 (its row is not in the matrix: clean, no count), cap + 1 wrong shares (failed, bytes kept), clean
  crossing list  item 0 dirty in every chunk, item 1 clean, the last item dirty in its first and last chunk and failed in one
                 in the middle: no count leaks from one item's summary into another's
  all n parties  every output equals zk_pss_repair_batch's byte for byte
  refusals       the list's (ZK_ERR_BAD_INPUT, ZK_ERR_PROTOCOL) and the batch's: shares and status untouched, the context
                 works afterwards
nchunks = 512 are two workgroups of the scan per item (four at l = 8), nchunks = 4 one partial workgroup.  At dimension 2l a
list of np parties corrects (np - 2l) // 2 wrong shares per chunk: l - 1 with n - 1 or n - 2 parties, so at l = 1 a list of 3
only detects."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk

from gpu_util import ctx
from test_gpu_repair_batch import CONFIGS, IDS, ITEMS, PAD, SIZES, _batch_buffer, _honest, _raw

BAD_INPUT, PROTOCOL = 4, 2


def _lists(n, l):
    """[(name, parties)]: all n; n - 1 with the first, a middle and the last party absent; for l >= 2, n - 2"""
    full = list(range(n))
    out = [("all", full)] + [("absent_%d" % e, [p for p in full if p != e]) for e in (0, n // 2, n - 1)]
    if l >= 2:
        out.append(("absent_1_%d" % (n - 2), [p for p in full if p not in (1, n - 2)]))
    return out


def _cap(S, dim):
    return (len(S) - dim) // 2


def _items(pp, S, nitems, nch, seed):
    """nitems compact matrices [|S|][nch][4] at dimension 2l: item i has a listed liar in every chunk when i % 4 == 0, a liar
    that is ABSENT when i % 4 == 1 (or, with all parties listed, is clean), cap + 1 wrong shares in its first and last chunk
    and cap in a middle one when i % 4 == 2, and is clean when i % 4 == 3"""
    rng = np.random.default_rng(seed)
    n, dim = pp.n, 2 * pp.l
    cap = _cap(S, dim)
    absent = [p for p in range(n) if p not in S]
    mats = []
    for i in range(nitems):
        m = _honest(pp, nch, dim, seed + 10 * (i % 2)).copy()
        if i % 4 == 0:
            m[S[(i + 1) % len(S)]] = _raw(rng, nch)
        elif i % 4 == 1:
            for p in absent:
                m[p] = _raw(rng, nch)
        elif i % 4 == 2:
            for c, cnt in ((0, cap + 1), (nch - 1, cap + 1), (nch // 2, cap)):
                for p in random.Random(seed + c + i).sample(S, cnt):
                    m[p, c] = _raw(rng)
        mats.append(np.ascontiguousarray(m[S]))
    return mats


def _single(pp, m, S, nch, dim):
    d = zk.DeviceBuffer.from_numpy(pp, m)
    r = pp.repair(d, nch, dim, parties=S)
    return d.to_numpy().reshape(m.shape), r.status_host().copy(), r.errpos_host().copy(), r.summary


def _check_against_singles(pp, S, mats, nch, dim, pad, what):
    nitems, per = len(mats), len(S) * nch
    host, stride = _batch_buffer(pp, mats, pad, np.random.default_rng(7))
    d = zk.DeviceBuffer.from_numpy(pp, host)
    r = pp.repair_batch(d, nitems, nch, dim, item_stride=stride, parties=S)
    assert r.parties == list(S) and r.out is d and r.nitems == nitems
    got = d.to_numpy().reshape(-1, 4)
    status, errpos = r.status_host().reshape(nitems, nch), r.errpos_host().reshape(nitems, nch)
    sums = r.summaries
    assert len(sums) == nitems, what
    seen = set()
    for i, m in enumerate(mats):
        w_sh, w_st, w_ep, w_sum = _single(pp, m, S, nch, dim)
        assert np.array_equal(got[i * stride:i * stride + per], w_sh.reshape(per, 4)), (what, i)
        assert np.array_equal(got[i * stride + per:(i + 1) * stride], host[i * stride + per:(i + 1) * stride]), (what, i)
        assert np.array_equal(status[i], w_st) and np.array_equal(errpos[i], w_ep), (what, i)
        assert sums[i] == w_sum and sum(w_sum[:3]) == nch, (what, i)
        seen |= set(int(s) for s in w_st)
    return seen, status, errpos, sums


# ---------------------------------------------------------------- against nitems single calls
@pytest.mark.parametrize("nitems", ITEMS)
@pytest.mark.parametrize("nch", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_batch_equals_the_single_calls(curve, l, nch, nitems):
    pp = ctx(curve, l)
    n, dim = pp.n, 2 * l
    for name, S in _lists(n, l):
        cap = _cap(S, dim)
        for pad in (0, PAD):
            mats = _items(pp, S, nitems, nch, 500 + l)
            what = (curve, l, nch, nitems, name, pad)
            seen, status, errpos, sums = _check_against_singles(pp, S, mats, nch, dim, pad, what)
            # the cases bite: a listed liar in every chunk of item 0 is named and repaired (found and failed where cap == 0)
            liar = S[1 % len(S)]
            if cap >= 1:
                assert (status[0] == 1).all() and (errpos[0] == 1 << liar).all(), what
                assert sums[0] == [0, nch, 0] + [nch if p == liar else 0 for p in range(n)], what
            else:
                assert (status[0] == 2).all() and not errpos[0].any() and sums[0] == [0, 0, nch] + [0] * n, what
            if nitems >= 3:
                # the absent liar: clean, the count stays 0; cap + 1 wrong shares: failed
                assert sums[1] == [nch, 0, 0] + [0] * n, what
                assert status[2][0] == 2 and status[2][nch - 1] == 2 and sums[2][2] >= 2, what
                assert seen == ({0, 1, 2} if cap >= 1 else {0, 2}), what


# ---------------------------------------------------------------- a dirty list that crosses items
@pytest.mark.parametrize("nitems", [3, 7])
@pytest.mark.parametrize("nch", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_a_dirty_list_that_crosses_items(curve, l, nch, nitems):
    pp = ctx(curve, l)
    n, dim = pp.n, 2 * l
    for name, S in _lists(n, l)[1:]:
        cap = _cap(S, dim)
        rng = np.random.default_rng(530 + l)
        honest = [np.ascontiguousarray(_honest(pp, nch, dim, 540 + i % 2)[S]) for i in range(nitems)]
        mats = [m.copy() for m in honest]
        rows = len(S)
        liar_row = rows // 2
        liar = S[liar_row]
        mats[0][liar_row] = _raw(rng, nch)                                  # item 0: one listed liar in every chunk
        last, mid = nitems - 1, (1 if nch == 4 else nch // 2)
        few = sorted(random.Random(l).sample(range(rows), max(cap, 1)))     # cap liars: corrected (one, failed, at cap 0)
        many = sorted(random.Random(l + 1).sample(range(rows), cap + 1))    # cap + 1: failed, bytes kept
        for c in (0, nch - 1):
            for r_ in few:
                mats[last][r_, c] = _raw(rng)
        for r_ in many:
            mats[last][r_, mid] = _raw(rng)
        for pad in (0, PAD):
            what = (curve, l, nch, nitems, name, pad)
            host, stride = _batch_buffer(pp, mats, pad, rng)
            d = zk.DeviceBuffer.from_numpy(pp, host)
            r = pp.repair_batch(d, nitems, nch, dim, item_stride=stride, parties=S)
            status, errpos = r.status_host().reshape(nitems, nch), r.errpos_host().reshape(nitems, nch)
            want_status, want_err = np.zeros((nitems, nch), np.uint8), np.zeros((nitems, nch), np.uint32)
            want_sums = [[nch, 0, 0] + [0] * n for _ in range(nitems)]
            fixed = [m.copy() for m in honest]
            fixed[last][:, mid] = mats[last][:, mid]
            if cap >= 1:
                want_status[0], want_err[0] = 1, 1 << liar
                want_status[last, [0, nch - 1]], want_err[last, [0, nch - 1]] = 1, sum(1 << S[r_] for r_ in few)
                want_sums[0] = [0, nch, 0] + [nch if p == liar else 0 for p in range(n)]
                want_sums[last] = [nch - 3, 2, 1] + [2 if p in [S[r_] for r_ in few] else 0 for p in range(n)]
            else:
                want_status[0] = 2
                want_status[last, [0, nch - 1]] = 2
                want_sums[0] = [0, 0, nch] + [0] * n
                want_sums[last] = [nch - 3, 0, 3] + [0] * n
                fixed[0] = mats[0]
                fixed[last] = mats[last]
            want_status[last, mid] = 2
            assert np.array_equal(status, want_status) and np.array_equal(errpos, want_err), what
            assert r.summaries == want_sums, what
            want, _ = _batch_buffer(pp, fixed, pad, rng)
            per = rows * nch
            got = d.to_numpy().reshape(-1, 4)
            for i in range(nitems):
                assert np.array_equal(got[i * stride:i * stride + per], want[i * stride:i * stride + per]), (what, i)
                assert np.array_equal(got[i * stride + per:(i + 1) * stride], host[i * stride + per:(i + 1) * stride])


# ---------------------------------------------------------------- all n parties: zk_pss_repair_batch
@pytest.mark.parametrize("nch", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_all_parties_listed_equals_repair_batch_byte_for_byte(curve, l, nch):
    pp = ctx(curve, l)
    n, dim, nitems = pp.n, 2 * l, 3
    full = list(range(n))
    mats = _items(pp, full, nitems, nch, 560 + l)
    host, stride = _batch_buffer(pp, mats, PAD, np.random.default_rng(9))
    ref_d = zk.DeviceBuffer.from_numpy(pp, host)
    ref = pp.repair_batch(ref_d, nitems, nch, dim, item_stride=stride)
    assert set(int(s) for s in ref.status_host()) == {0, 1, 2}
    fn = pp.lib.zk_pss_repair_batch_parties
    for ids in (None, (C.c_uint32 * n)(*full)):
        d = zk.DeviceBuffer.from_numpy(pp, host)
        st, ep = zk.DeviceBuffer(pp, nitems * nch), zk.DeviceBuffer(pp, 4 * nitems * nch)
        sm = zk.DeviceBuffer(pp, 8 * (3 + n) * nitems)
        pp._check(fn(pp.h, d.ptr, ids, n, stride, nitems, nch, dim, st.ptr, ep.ptr, sm.ptr, None))
        for a, b in ((st, ref.status), (ep, ref.errpos), (sm, ref.summary_d), (d, ref_d)):
            assert np.array_equal(a.to_numpy(np.uint8), b.to_numpy(np.uint8)), (curve, l, nch)


# ---------------------------------------------------------------- one item: zk_pss_repair_parties; no errpos, no summary
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_one_item_without_errpos_and_summary(curve, l):
    pp = ctx(curve, l)
    n, dim, nch = pp.n, 2 * l, 4
    S = [p for p in range(n) if p != n // 2]
    m = _items(pp, S, 3, nch, 570 + l)[2]
    w_sh, w_st, _, _ = _single(pp, m, S, nch, dim)
    d, st = zk.DeviceBuffer.from_numpy(pp, m), zk.DeviceBuffer(pp, nch)
    ids = (C.c_uint32 * len(S))(*S)
    pp._check(pp.lib.zk_pss_repair_batch_parties(pp.h, d.ptr, ids, len(S), len(S) * nch, 1, nch, dim, st.ptr, None, None, None))
    assert np.array_equal(d.to_numpy().reshape(m.shape), w_sh) and np.array_equal(st.to_numpy(np.uint8), w_st)


# ---------------------------------------------------------------- refusals
def test_refusals_write_nothing_and_the_context_works_afterwards():
    pp = ctx("bn254", 2)
    n, nch, dim = pp.n, 4, 4
    S = [0, 1, 2, 3, 5, 6, 7]
    np_ = len(S)
    mats = _items(pp, S, 3, nch, 580)
    host, stride = _batch_buffer(pp, mats, 0, np.random.default_rng(8))
    d = zk.DeviceBuffer.from_numpy(pp, host)
    st = zk.DeviceBuffer.from_numpy(pp, np.full(3 * nch, 0xAB, np.uint8))
    arr = lambda s: (C.c_uint32 * len(s))(*s)
    call = lambda sh, ids, cnt, stride_, items, chunks, k, status: pp.lib.zk_pss_repair_batch_parties(
        pp.h, sh, ids, cnt, stride_, items, chunks, k, status, None, None, None)
    for what, want, rc in (
            ("no items", BAD_INPUT, call(d.ptr, arr(S), np_, stride, 0, nch, dim, st.ptr)),
            ("negative items", BAD_INPUT, call(d.ptr, arr(S), np_, stride, -1, nch, dim, st.ptr)),
            ("too many items", BAD_INPUT, call(d.ptr, arr(S), np_, stride, 49, nch, dim, st.ptr)),
            ("stride below nparties * nchunks", BAD_INPUT, call(d.ptr, arr(S), np_, np_ * nch - 1, 3, nch, dim, st.ptr)),
            ("2^32 entries", BAD_INPUT, call(d.ptr, arr(S), np_, np_ << 31, 2, 1 << 31, dim, st.ptr)),
            ("2^32 chunks", BAD_INPUT, call(d.ptr, arr(S), np_, np_ << 32, 1, 1 << 32, dim, st.ptr)),
            ("dimension 0", BAD_INPUT, call(d.ptr, arr(S), np_, stride, 3, nch, 0, st.ptr)),
            ("dimension n", BAD_INPUT, call(d.ptr, arr(S), np_, stride, 3, nch, n, st.ptr)),
            ("null shares", BAD_INPUT, call(None, arr(S), np_, stride, 3, nch, dim, st.ptr)),
            ("null status", BAD_INPUT, call(d.ptr, arr(S), np_, stride, 3, nch, dim, None)),
            ("no parties", BAD_INPUT, call(d.ptr, arr(S), 0, stride, 3, nch, dim, st.ptr)),
            ("more than n parties", BAD_INPUT, call(d.ptr, arr(S + [8, 9]), n + 1, stride, 3, nch, dim, st.ptr)),
            ("an unsorted list", BAD_INPUT, call(d.ptr, arr([0, 1, 3, 2, 5, 6, 7]), np_, stride, 3, nch, dim, st.ptr)),
            ("a repeated id", BAD_INPUT, call(d.ptr, arr([0, 1, 2, 2, 5, 6, 7]), np_, stride, 3, nch, dim, st.ptr)),
            ("an id >= n", BAD_INPUT, call(d.ptr, arr([0, 1, 2, 3, 5, 6, 8]), np_, stride, 3, nch, dim, st.ptr)),
            ("nparties == dimension", PROTOCOL, call(d.ptr, arr(S[:dim]), dim, stride, 3, nch, dim, st.ptr)),
            ("nparties < dimension", PROTOCOL, call(d.ptr, arr(S[:2]), 2, stride, 3, nch, dim, st.ptr))):
        assert rc == want, what
        assert np.array_equal(d.to_numpy().reshape(-1, 4), host) and (st.to_numpy(np.uint8) == 0xAB).all(), what
    assert call(None, arr(S), np_, 0, 3, 0, dim, None) == 0                # nchunks == 0 is ZK_OK
    assert (st.to_numpy(np.uint8) == 0xAB).all()
    _check_against_singles(pp, S, mats, nch, dim, 0, "after the refusals")
