"""GPU tests (through the C ABI) for zk_pss_repair_batch: zk_pss_repair of several share matrices, item i at
shares_d + i * item_stride, with one scan launch (the item on grid.y) and one decoder launch over ONE list of dirty
(item, chunk) entries.
  yardstick      nitems calls of zk_pss_repair on copies of the same matrices: shares, status, errpos and summary are equal
                 byte for byte, per item; the pad between two items keeps its bytes
  crossing list  item 0 dirty in every chunk, item 1 clean, the last item dirty in its first and last chunk and failed in one
                 in the middle: no count leaks from one item's summary into another's
  refusals       ZK_ERR_BAD_INPUT, shares and status untouched, the context works afterwards
nchunks = 512 are two workgroups of the scan per item (four at l = 8), nchunks = 4 one partial workgroup; dimension 2l corrects
up to l wrong shares, 4l - 1 only detects."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk

from gpu_util import ctx

CONFIGS = [("bn254", 1), ("bn254", 2), ("bn254", 4), ("bn254", 8), ("bls12_381", 2), ("bls12_377", 2)]
IDS = ["%s_l%d" % c for c in CONFIGS]
SIZES = [512, 4]
ITEMS = [1, 3, 7]
PAD = 5                      # elements between two items of a padded batch
BAD_INPUT = 4


def _raw(rng, *shape):
    """random field elements as limbs: anything below 2^252 is one, in Montgomery form, for all three scalar fields"""
    a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


_words = {}


def _honest(pp, nch, dim, seed):
    """a matrix [n][nch][4] of codewords of the given dimension: packed shares (2l), or products of two (4l - 1).  Computed
    once per shape and never changed: the callers copy."""
    key = (pp.curve, pp.l, nch, dim, seed)
    if key not in _words:
        def packed(s):
            sec = zk.DeviceBuffer.from_numpy(pp, _raw(np.random.default_rng(s), nch * pp.l))
            return pp.pack(sec, nch, seed=s)
        if dim == 2 * pp.l:
            out = packed(seed)
        else:
            a, b = packed(seed), packed(seed + 1)
            zero = zk.DeviceBuffer.from_numpy(pp, np.zeros((pp.n * nch, 4), np.uint64))
            out = pp.alloc_fr(pp.n * nch)
            pp._check(pp.lib.zk_vec_mul_sub(pp.h, out.ptr, a.ptr, b.ptr, zero.ptr, pp.n * nch, None))
        _words[key] = out.to_numpy().reshape(pp.n, nch, 4).copy()
    return _words[key]


def _cap(pp, dim):
    return (pp.n - dim) // 2


def _items(pp, nitems, nch, dim, seed):
    """nitems matrices with errors of every kind: item i has a liar in every chunk when i % 3 == 0, is clean when
    i % 3 == 1, and otherwise has cap wrong shares in chunk 0, cap + 1 in the last chunk and one in a middle chunk"""
    rng = np.random.default_rng(seed)
    cap = _cap(pp, dim)
    mats = []
    for i in range(nitems):
        m = _honest(pp, nch, dim, seed + 10 * (i % 2)).copy()
        if i % 3 == 0:
            m[(i + 1) % pp.n] = _raw(rng, nch)
        elif i % 3 == 2:
            for c, cnt in ((0, max(cap, 1)), (nch - 1, cap + 1), (nch // 2, 1)):
                for p in random.Random(seed + c + i).sample(range(pp.n), cnt):
                    m[p, c] = _raw(rng)
        mats.append(m)
    return mats


def _batch_buffer(pp, mats, pad, rng):
    """the matrices at a stride of n * nch + pad elements, random bytes in the pads -> (host array [total][4], stride)"""
    per = mats[0].shape[0] * mats[0].shape[1]
    stride = per + pad
    buf = _raw(rng, stride * len(mats))
    for i, m in enumerate(mats):
        buf[i * stride:i * stride + per] = m.reshape(per, 4)
    return buf, stride


def _single(pp, m, nch, dim):
    d = zk.DeviceBuffer.from_numpy(pp, m)
    r = pp.repair(d, nch, dim)
    return d.to_numpy().reshape(m.shape), r.status_host().copy(), r.errpos_host().copy(), r.summary


def _check_against_singles(pp, mats, nch, dim, pad, what):
    nitems, per = len(mats), pp.n * nch
    host, stride = _batch_buffer(pp, mats, pad, np.random.default_rng(7))
    d = zk.DeviceBuffer.from_numpy(pp, host)
    r = pp.repair_batch(d, nitems, nch, dim, item_stride=stride)
    got = d.to_numpy().reshape(-1, 4)
    status, errpos = r.status_host().reshape(nitems, nch), r.errpos_host().reshape(nitems, nch)
    sums = r.summaries
    assert len(sums) == nitems, what
    seen = set()
    for i, m in enumerate(mats):
        w_sh, w_st, w_ep, w_sum = _single(pp, m, nch, dim)
        assert np.array_equal(got[i * stride:i * stride + per], w_sh.reshape(per, 4)), (what, i)
        assert np.array_equal(got[i * stride + per:(i + 1) * stride], host[i * stride + per:(i + 1) * stride]), (what, i)
        assert np.array_equal(status[i], w_st) and np.array_equal(errpos[i], w_ep), (what, i)
        assert sums[i] == w_sum and sum(w_sum[:3]) == nch, (what, i)
        seen |= set(int(s) for s in w_st)
    return seen


# ---------------------------------------------------------------- against nitems single calls
@pytest.mark.parametrize("nitems", ITEMS)
@pytest.mark.parametrize("nch", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_batch_equals_the_single_calls(curve, l, nch, nitems):
    pp = ctx(curve, l)
    for dim in (2 * l, 4 * l - 1):
        for pad in (0, PAD):
            seen = _check_against_singles(pp, _items(pp, nitems, nch, dim, 400 + l), nch, dim, pad, (curve, l, nch, nitems, dim, pad))
            # the cases bite: at dimension 2l a batch of three holds clean, corrected and failed chunks
            if nitems >= 3:
                assert seen == ({0, 1, 2} if dim == 2 * l else {0, 2})


@pytest.mark.parametrize("nch", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_one_item_equals_zk_pss_repair(curve, l, nch):
    pp = ctx(curve, l)
    for dim in (2 * l, 4 * l - 1):
        m = _items(pp, 3, nch, dim, 420 + l)[2]
        w_sh, w_st, w_ep, w_sum = _single(pp, m, nch, dim)
        d = zk.DeviceBuffer.from_numpy(pp, m)
        r = pp.repair_batch(d, 1, nch, dim)
        assert np.array_equal(d.to_numpy().reshape(m.shape), w_sh), (curve, l, nch, dim)
        assert np.array_equal(r.status_host(), w_st) and np.array_equal(r.errpos_host(), w_ep), (curve, l, nch, dim)
        assert r.summary == w_sum and r.summaries == [w_sum], (curve, l, nch, dim)
        # without errpos and summary the shares and the status are the same
        d2, st = zk.DeviceBuffer.from_numpy(pp, m), zk.DeviceBuffer(pp, nch)
        pp._check(pp.lib.zk_pss_repair_batch(pp.h, d2.ptr, pp.n * nch, 1, nch, dim, st.ptr, None, None, None))
        assert np.array_equal(d2.to_numpy().reshape(m.shape), w_sh) and np.array_equal(st.to_numpy(np.uint8), w_st)


# ---------------------------------------------------------------- a dirty list that crosses items
@pytest.mark.parametrize("nitems", [3, 7])
@pytest.mark.parametrize("nch", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_a_dirty_list_that_crosses_items(curve, l, nch, nitems):
    pp = ctx(curve, l)
    n, dim = pp.n, 2 * l
    rng = np.random.default_rng(430 + l)
    honest = [_honest(pp, nch, dim, 440 + i % 2) for i in range(nitems)]
    mats = [m.copy() for m in honest]
    liar = n // 2
    mats[0][liar] = _raw(rng, nch)                                      # item 0: one liar in every chunk
    last, mid = nitems - 1, (1 if nch == 4 else nch // 2)
    few = sorted(random.Random(l).sample(range(n), l))                  # l liars: corrected
    many = sorted(random.Random(l + 1).sample(range(n), l + 1))         # l + 1: failed, bytes kept
    for c in (0, nch - 1):
        for p in few:
            mats[last][p, c] = _raw(rng)
    for p in many:
        mats[last][p, mid] = _raw(rng)
    for pad in (0, PAD):
        host, stride = _batch_buffer(pp, mats, pad, rng)
        d = zk.DeviceBuffer.from_numpy(pp, host)
        r = pp.repair_batch(d, nitems, nch, dim, item_stride=stride)
        status, errpos = r.status_host().reshape(nitems, nch), r.errpos_host().reshape(nitems, nch)
        want_status, want_err = np.zeros((nitems, nch), np.uint8), np.zeros((nitems, nch), np.uint32)
        want_status[0], want_err[0] = 1, 1 << liar
        want_status[last, [0, nch - 1]], want_err[last, [0, nch - 1]] = 1, sum(1 << p for p in few)
        want_status[last, mid] = 2
        assert np.array_equal(status, want_status) and np.array_equal(errpos, want_err), (curve, l, nch, nitems, pad)
        want_sums = [[nch, 0, 0] + [0] * n for _ in range(nitems)]
        want_sums[0] = [0, nch, 0] + [nch if p == liar else 0 for p in range(n)]
        want_sums[last] = [nch - 3, 2, 1] + [2 if p in few else 0 for p in range(n)]
        assert r.summaries == want_sums, (curve, l, nch, nitems, pad)
        fixed = [m.copy() for m in honest]
        fixed[last][:, mid] = mats[last][:, mid]
        want, _ = _batch_buffer(pp, fixed, pad, rng)
        per = n * nch
        got = d.to_numpy().reshape(-1, 4)
        for i in range(nitems):
            assert np.array_equal(got[i * stride:i * stride + per], want[i * stride:i * stride + per]), (curve, l, nch, i)
            assert np.array_equal(got[i * stride + per:(i + 1) * stride], host[i * stride + per:(i + 1) * stride])


# ---------------------------------------------------------------- refusals
def test_refusals_write_nothing_and_the_context_works_afterwards():
    pp = ctx("bn254", 2)
    n, nch, dim = pp.n, 4, 4
    mats = _items(pp, 3, nch, dim, 450)
    host, stride = _batch_buffer(pp, mats, 0, np.random.default_rng(8))
    d = zk.DeviceBuffer.from_numpy(pp, host)
    st = zk.DeviceBuffer.from_numpy(pp, np.full(3 * nch, 0xAB, np.uint8))
    call = lambda sh, stride_, items, chunks, k, status: pp.lib.zk_pss_repair_batch(
        pp.h, sh, stride_, items, chunks, k, status, None, None, None)
    for what, rc in (("no items", call(d.ptr, stride, 0, nch, dim, st.ptr)),
                     ("negative items", call(d.ptr, stride, -1, nch, dim, st.ptr)),
                     ("too many items", call(d.ptr, stride, 49, nch, dim, st.ptr)),
                     ("stride below n * nchunks", call(d.ptr, n * nch - 1, 3, nch, dim, st.ptr)),
                     ("2^32 entries", call(d.ptr, n << 31, 2, 1 << 31, dim, st.ptr)),
                     ("2^32 chunks", call(d.ptr, n << 32, 1, 1 << 32, dim, st.ptr)),
                     ("dimension 0", call(d.ptr, stride, 3, nch, 0, st.ptr)),
                     ("dimension n", call(d.ptr, stride, 3, nch, n, st.ptr)),
                     ("null shares", call(None, stride, 3, nch, dim, st.ptr)),
                     ("null status", call(d.ptr, stride, 3, nch, dim, None))):
        assert rc == BAD_INPUT, what
        assert np.array_equal(d.to_numpy().reshape(-1, 4), host) and (st.to_numpy(np.uint8) == 0xAB).all(), what
    assert call(None, 0, 3, 0, dim, None) == 0                           # nchunks == 0 is ZK_OK
    assert (st.to_numpy(np.uint8) == 0xAB).all()
    _check_against_singles(pp, mats, nch, dim, 0, "after the refusals")
