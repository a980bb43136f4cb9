"""GPU tests (through the C ABI) for zk_circom_h_batch_checked: the checked h chain of a batch of proofs as one launch chain.
CONTRACT: proof b of the batch is zk_circom_h_checked with seed + 16 b -- h bit for bit, and the slice of proof b in the
proof-major report ([nb][7][m/l] status and errpos, [nb][7][3 + n] summaries) byte for byte what that single call writes.
Random share vectors, no circuit.  Every case compares each proof of the batch with
  * zk_circom_h_checked(seed + 16 b) on the same input: h, status, errpos and all 7 summary rows, and
  * zk_circom_h(seed + 16 b) on the HONEST input: a liar of items 0..2 is corrected, so h stays the honest h,
and then states the report it expects in numbers.
  clean           nb = 1, 2, 3, 16 (16 proofs are the 48 items one repair call and one king launch take)
  one liar        nb = 3, party p's rows of qap_a, qap_b, qap_c of proof 1 replaced: proof 1's items 0..2 name p in every
                  chunk, every other row of every proof is clean
  two liars       p0 in proof 0, p2 in proof 2: each report names its own liar (an item / proof mix-up in the gather)
  masks           none at all; in-masks in round 1 only; mask sets that differ between the proofs (the proof-by-proof route)
  partial masks   nb = 2, on every proof the in-masks of items 1, 3 and 4 absent: alike across the batch, not within a round,
                  so the proofs run one by one and their kings item by item; clean and with one liar; bn254 l = 2 and l = 8
                  at m/l = 4 (one partial workgroup of the scan) and 512 (two per item, four at l = 8)
  optional        errpos_d and summary_d NULL: same statuses, same h
  refusals        nb = 0, nb = 17, null pointers: ZK_ERR_BAD_INPUT, the report buffers keep their sentinel bytes
Sizes: m/l half of, and twice, the number of chunks one workgroup of the repair's scan takes (GAO_THREADS of gao_impl.hpp at
l <= 4, where a chunk is one lane group's): one partial workgroup per item, and two."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import api
from zksaas_amd import groth16 as zg

from gpu_util import ctx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAO_THREADS = int(re.search(r"constexpr int GAO_THREADS = (\d+);",
                            open(os.path.join(ROOT, "zk-saas_amd", "csrc", "gao_impl.hpp")).read()).group(1))
CONFIGS = [("bn254", 1), ("bn254", 2), ("bn254", 4), ("bls12_381", 2)]
IDS = ["%s_l%d" % c for c in CONFIGS]
SIZES = [GAO_THREADS // 2, GAO_THREADS * 2]
BAD_INPUT = 4
SEED = 91
STEP = 16                     # PROOF_SEED_STEP
NSETS = 3                     # distinct mask sets; proof b of a larger batch takes set b % NSETS


def _raw(rng, *shape):
    """random field elements as limbs: anything below 2^252 is one, in Montgomery form, for the scalar fields used here"""
    a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


def _log_m(pp, Lc):
    return (Lc * pp.l).bit_length() - 1


def _dev(pp, arr):
    return zk.DeviceBuffer.from_numpy(pp, arr)


_qap, _masks, _single = {}, {}, {}


def _honest(pp, Lc, b):
    """the three matrices [n][Lc][4] of packed shares of proof b: made once, never changed"""
    key = (pp.curve, pp.l, Lc, b)
    if key not in _qap:
        rows = []
        for k in range(3):
            sec = _dev(pp, _raw(np.random.default_rng(700 + 3 * b + k), Lc * pp.l))
            rows.append(pp.pack(sec, Lc, seed=760 + 3 * b + k).to_numpy().reshape(pp.n, Lc, 4).copy())
        _qap[key] = rows
    return _qap[key]


def _copy_masks(ct):
    mk = zg.Masks()
    C.memmove(C.byref(mk), C.byref(ct), C.sizeof(zg.Masks))
    return mk


def _mask_set(pp, Lc, b, which):
    """the zk_groth16_masks of proof b (None: no masks).  The dealt buffers are shared among the tests and never written.
    all: all twelve masks; round1: no in-masks in the d_fft round; mixed: proof 1 lacks the in-mask of item 0; partial: every
    proof lacks those of items 1, 3 and 4 (the set of test_gpu_circom_h_checked.py)"""
    if which == "none":
        return None
    key = (pp.curve, pp.l, Lc, b % NSETS)
    if key not in _masks:
        _masks[key] = zg.ProofMasks(pp, _log_m(pp, Lc), 800 + STEP * (b % NSETS))
    mk = _copy_masks(_masks[key].ct)
    if which == "round1":
        for k in (3, 4, 5):
            mk.fft_in[k] = None
    if which == "mixed" and b == 1:
        mk.fft_in[0] = None
    if which == "partial":
        for k in (1, 3, 4):                     # round 1: a and c masked; round 2: c only
            mk.fft_in[k] = None
    return mk


def _liar(rows, p, seed):
    """party p's rows of the three matrices replaced"""
    out = []
    for k, r in enumerate(rows):
        cur = r.copy()
        cur[p] = _raw(np.random.default_rng(seed + k), r.shape[1])
        out.append(cur)
    return out


def _single_calls(pp, Lc, b, which, rows=None):
    """(h of zk_circom_h, h / status / errpos / summaries of zk_circom_h_checked) of proof b alone with seed + 16 b; the
    honest input's are computed once"""
    key = (pp.curve, pp.l, Lc, b, which)
    if rows is None and key in _single:
        return _single[key]
    cur = _honest(pp, Lc, b) if rows is None else rows
    mk, log_m, seed = _mask_set(pp, Lc, b, which), _log_m(pp, Lc), SEED + STEP * b
    h0 = api.circom_h(pp, [_dev(pp, r) for r in cur], mk, seed, log2_m=log_m).to_numpy()
    h1, rep = api.circom_h(pp, [_dev(pp, r) for r in cur], mk, seed, check=True, log2_m=log_m)
    res = (h0, h1.to_numpy(), rep.status_host().copy(), rep.errpos_host().copy(), rep.summaries)
    if rows is None:
        _single[key] = res
    return res


def _summary(pp, Lc, status, parties=()):
    s = [0] * (3 + pp.n)
    s[status] = Lc
    for p in parties:
        s[3 + p] = Lc
    return s


def _batch(pp, Lc, nb, which, liars=None, **kw):
    """runs the batch (liars: {proof: party}) and checks every proof against the single calls; returns the reports"""
    liars = liars or {}
    rows = [_liar(_honest(pp, Lc, b), liars[b], 900 + 10 * b) if b in liars else _honest(pp, Lc, b) for b in range(nb)]
    bufs = [[_dev(pp, r) for r in rows[b]] for b in range(nb)]
    masks = None if which == "none" else [_mask_set(pp, Lc, b, which) for b in range(nb)]
    hs, reps = api.circom_h_batch_checked(pp, bufs, masks, SEED, log2_m=_log_m(pp, Lc), **kw)
    assert len(hs) == nb and len(reps) == nb
    for b in range(nb):
        tag = (pp.curve, pp.l, Lc, nb, which, b)
        honest_h = _single_calls(pp, Lc, b, which)[0]
        _, h1, st, ep, sm = _single_calls(pp, Lc, b, which, rows[b] if b in liars else None)
        got = hs[b].to_numpy()
        assert np.array_equal(got, h1), tag                               # the single checked call, bit for bit
        assert np.array_equal(got, honest_h), tag                          # the honest h: a liar is corrected
        assert np.array_equal(reps[b].status_host(), st), tag
        if kw.get("errpos", True):
            assert np.array_equal(reps[b].errpos_host(), ep), tag
        if kw.get("summary", True):
            assert reps[b].summaries == sm and len(sm) == 7, tag
        # and in numbers
        want_st, want_ep = np.zeros((7, Lc), np.uint8), np.zeros((7, Lc), np.uint32)
        want_sm = [_summary(pp, Lc, 0)] * 7
        if b in liars:
            want_st[:3], want_ep[:3] = 1, 1 << liars[b]
            want_sm = [_summary(pp, Lc, 1, [liars[b]])] * 3 + want_sm[3:]
        assert np.array_equal(reps[b].status_host().reshape(7, Lc), want_st), tag
        if kw.get("errpos", True):
            assert np.array_equal(reps[b].errpos_host().reshape(7, Lc), want_ep), tag
        if kw.get("summary", True):
            assert reps[b].summaries == want_sm, tag
    return reps


@pytest.mark.parametrize("nb", [1, 2, 3, 16])
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_clean_batch_is_the_single_calls(curve, l, Lc, nb):
    _batch(ctx(curve, l), Lc, nb, "all")


@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_one_liar_in_one_proof(curve, l, Lc):
    pp = ctx(curve, l)
    _batch(pp, Lc, 3, "all", {1: pp.n - 2})


@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_different_liars_in_different_proofs(curve, l, Lc):
    pp = ctx(curve, l)
    _batch(pp, Lc, 3, "all", {0: 1, 2: pp.n - 1})


@pytest.mark.parametrize("which", ["none", "round1", "mixed"])
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_mask_sets(curve, l, Lc, which):
    pp = ctx(curve, l)
    _batch(pp, Lc, 3, which)
    _batch(pp, Lc, 3, which, {1: pp.n - 2})
    _batch(pp, Lc, 3, which, {0: 1, 2: pp.n - 1})


@pytest.mark.parametrize("Lc", [4, 512])
@pytest.mark.parametrize("l", [2, 8])
def test_masks_partial_within_a_round_alike_across_the_batch(l, Lc):
    pp = ctx("bn254", l)
    _batch(pp, Lc, 2, "partial")
    _batch(pp, Lc, 2, "partial", {1: pp.n - 2})


@pytest.mark.parametrize("Lc", SIZES)
def test_errpos_and_summary_are_optional(Lc):
    pp = ctx("bn254", 2)
    _batch(pp, Lc, 3, "all", {1: 3}, errpos=False, summary=False)
    _batch(pp, Lc, 3, "mixed", {1: 3}, errpos=False, summary=False)


def test_refusals():
    pp = ctx("bn254", 2)
    Lc, log_m = SIZES[0], _log_m(ctx("bn254", 2), SIZES[0])
    bufs = [[_dev(pp, r) for r in _honest(pp, Lc, b)] for b in range(17)]
    h = pp.alloc_fr(17 * pp.n * Lc)
    st = _dev(pp, np.full(17 * 7 * Lc, 0xAB, np.uint8))
    ep = _dev(pp, np.full(17 * 7 * Lc, 0xABABABAB, np.uint32))
    sm = _dev(pp, np.full(17 * 7 * (3 + pp.n), 0xABABABABABABABAB, np.uint64))
    hb = h.to_numpy().copy()
    arr = lambda k, nb, hole=None: (C.c_void_p * 17)(*[None if b == hole else bufs[b][k].ptr for b in range(17)])
    call = lambda nb, qa, qb, qc, lm, out, status: pp.lib.zk_circom_h_batch_checked(pp.h, nb, qa, qb, qc, lm, None, SEED, out,
                                                                                    status, ep.ptr, sm.ptr, None)
    a, b_, c = arr(0, 17), arr(1, 17), arr(2, 17)
    for what, rc in (("nb = 0", call(0, a, b_, c, log_m, h.ptr, st.ptr)), ("nb = 17", call(17, a, b_, c, log_m, h.ptr, st.ptr)),
                     ("nb = -1", call(-1, a, b_, c, log_m, h.ptr, st.ptr)),
                     ("null array", call(3, None, b_, c, log_m, h.ptr, st.ptr)),
                     ("null entry", call(3, a, arr(1, 17, hole=2), c, log_m, h.ptr, st.ptr)),
                     ("null h", call(3, a, b_, c, log_m, None, st.ptr)), ("null status", call(3, a, b_, c, log_m, h.ptr, None)),
                     ("m < l", call(3, a, b_, c, 0, h.ptr, st.ptr)), ("domain too large", call(3, a, b_, c, 28, h.ptr, st.ptr))):
        assert rc == BAD_INPUT, what
        assert np.array_equal(h.to_numpy(), hb), what
        assert (st.to_numpy(np.uint8) == 0xAB).all() and (ep.to_numpy(np.uint32) == 0xABABABAB).all(), what
        assert (sm.to_numpy(np.uint64) == 0xABABABABABABABAB).all(), what
    # the context is still usable
    _batch(pp, Lc, 2, "none")
