"""GPU tests (through the C ABI) for zk_circom_h_checked_parties: zk_circom_h_checked when only the listed parties' words reach
the kings -- all n parties or n - 1 of them.
  (a) honest input, n - 1 parties: h is bit for bit zk_circom_h's under the same seed and masks, items 0..5 are clean and
      item 6 is the all-zero "not checked" row (status and errpos bytes 0, summary all zeros)
  (b) the absent party's rows of the three QAP vectors and of all seven in-masks overwritten with random field elements: h is
      still bit-equal; on the same input the all-parties zk_circom_h_checked names that party in items 0..2 and in every
      masked item of 3..5 -- the input bites
  (c) a second liar beside the absent party (l >= 2: a list of n - 1 corrects l - 1 per chunk) is named by its id, h is honest
  (d) nparties == n equals zk_circom_h_checked in every output
  (e) refusals: a short list, an unsorted list, an id >= n, a null status -- nothing written
m / l = 512 chunks are two workgroups of the scan per item (four at l = 8), m / l = 4 is one partial workgroup.  Mask sets: all
twelve masks, none, and the in-masks of both rounds partly present (the kings then run item by item)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import api

from gpu_util import ctx
from test_gpu_circom_h_checked import (CONFIGS, IDS, MASK_SETS, SEED, SIZES, _dev, _h, _honest, _item_state, _liars, _log_m,
                                       _mask_set, _summary, _tampered_mask)

BAD_INPUT, PROTOCOL = 4, 2


def _without(pp, e):
    return [p for p in range(pp.n) if p != e]


def _h_list(pp, rows, mk, Lc, S):
    bufs = [_dev(pp, r) for r in rows]
    h, rep = api.circom_h(pp, bufs, mk, SEED, check=True, log2_m=_log_m(pp, Lc), parties=S)
    assert rep.parties == list(S)
    return h.to_numpy(), rep


def _unchecked_row(pp, rep, Lc):
    """item 6 with n - 1 parties: bytes 0 and an all-zero summary -- zero chunks checked"""
    st, ep = rep.status_host().reshape(7, Lc), rep.errpos_host().reshape(7, Lc)
    return not st[6].any() and not ep[6].any() and rep.summaries[6] == [0] * (3 + pp.n)


def _poisoned(pp, rows, mk, Lc, e, seed):
    """party e's rows of the QAP vectors and of every in-mask present replaced -> (rows, masks, buffers to keep)"""
    cur = [_liars(r, [e], seed + 10 * k) for k, r in enumerate(rows)]
    keep = []
    if mk is not None:
        for k in range(6):
            if mk.fft_in[k]:
                mk, buf = _tampered_mask(pp, mk, "fft_in", k, e, seed + 100 + k, Lc)
                keep.append(buf)
        if mk.degred_in:
            mk, buf = _tampered_mask(pp, mk, "degred_in", None, e, seed + 200, Lc)
            keep.append(buf)
    return cur, mk, keep


# ---------------------------------------------------------------- (a) (b): honest and poisoned input, one party absent
@pytest.mark.parametrize("which", MASK_SETS)
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_h_of_n_minus_1_parties_is_the_honest_h_whatever_the_absent_rows_hold(curve, l, Lc, which):
    pp = ctx(curve, l)
    rows, mk = _honest(pp, Lc), _mask_set(pp, Lc, which)
    want, _ = _h(pp, rows, mk, Lc, False)
    for e in (0, pp.n // 2, pp.n - 1):
        what = (curve, l, Lc, which, e)
        S = _without(pp, e)
        got, rep = _h_list(pp, rows, mk, Lc, S)
        assert np.array_equal(got, want), what
        assert _item_state(rep, Lc)[:6] == [(0, 0)] * 6 and rep.summaries[:6] == [_summary(pp, Lc, 0)] * 6, what
        assert _unchecked_row(pp, rep, Lc), what
        cur, bad, keep = _poisoned(pp, rows, mk, Lc, e, 600 + e)
        got, rep = _h_list(pp, cur, bad, Lc, S)
        assert np.array_equal(got, want), what
        assert _item_state(rep, Lc)[:6] == [(0, 0)] * 6 and rep.summaries[:6] == [_summary(pp, Lc, 0)] * 6, what
        assert _unchecked_row(pp, rep, Lc), what
        # the input bites: with all parties the checked chain names e wherever its row entered a word
        _, full = _h(pp, cur, bad, Lc, True)
        named = [True] * 3 + [bad is not None and bool(bad.fft_in[3 + k]) for k in range(3)]
        assert _item_state(full, Lc)[:6] == [(1, 1 << e) if b else (0, 0) for b in named], what
        del keep


# ---------------------------------------------------------------- (c): a second liar beside the absent party
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", [c for c in CONFIGS if c[1] >= 2], ids=[i for c, i in zip(CONFIGS, IDS) if c[1] >= 2])
def test_a_listed_liar_beside_the_absent_party_is_named(curve, l, Lc):
    pp = ctx(curve, l)
    rows = _honest(pp, Lc)
    for which in ("all", "partial"):
        mk = _mask_set(pp, Lc, which)
        want, _ = _h(pp, rows, mk, Lc, False)
        for e, q in ((0, pp.n - 1), (pp.n // 2, pp.n // 2 - 1), (pp.n - 1, 0)):
            what = (curve, l, Lc, which, e, q)
            cur, bad, keep = _poisoned(pp, rows, mk, Lc, e, 640 + e)
            cur = [_liars(cur[0], [q], 650), cur[1], _liars(cur[2], [q], 660)]
            got, rep = _h_list(pp, cur, bad, Lc, _without(pp, e))
            assert np.array_equal(got, want), what
            assert _item_state(rep, Lc)[:6] == [(1, 1 << q), (0, 0), (1, 1 << q)] + [(0, 0)] * 3, what
            assert rep.summaries[0] == _summary(pp, Lc, 1, [q]) and rep.summaries[1] == _summary(pp, Lc, 0), what
            assert _unchecked_row(pp, rep, Lc), what
            del keep


# ---------------------------------------------------------------- (d): all n parties listed
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_all_parties_listed_equals_circom_h_checked(curve, l, Lc):
    pp = ctx(curve, l)
    n = pp.n
    rows, mk = _honest(pp, Lc), _mask_set(pp, Lc, "all")
    cur = [_liars(rows[0], [n - 1], 670), rows[1], rows[2]]
    bad, keep = _tampered_mask(pp, mk, "degred_in", None, 1, 680, Lc)
    want, ref = _h(pp, cur, bad, Lc, True)
    assert _item_state(ref, Lc) == [(1, 1 << (n - 1))] + [(0, 0)] * 5 + [(2, 0)]
    fn = pp.lib.zk_circom_h_checked_parties
    for ids in (None, (C.c_uint32 * n)(*range(n))):
        bufs, h = [_dev(pp, r) for r in cur], pp.alloc_fr(n * Lc)
        rep = api.h_report(pp, _log_m(pp, Lc))
        pp._check(fn(pp.h, ids, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, _log_m(pp, Lc), C.byref(bad), SEED, h.ptr,
                     rep.status.ptr, rep.errpos.ptr, rep.summary_d.ptr, None))
        assert np.array_equal(h.to_numpy(), want), (curve, l, Lc)
        for a, b in ((rep.status, ref.status), (rep.errpos, ref.errpos), (rep.summary_d, ref.summary_d)):
            assert np.array_equal(a.to_numpy(np.uint8), b.to_numpy(np.uint8)), (curve, l, Lc)
    del keep


# ---------------------------------------------------------------- (e): refusals
def test_refusals_write_nothing():
    pp = ctx("bn254", 2)
    n, Lc = pp.n, 4
    rows = _honest(pp, Lc)
    bufs, h = [_dev(pp, r) for r in rows], pp.alloc_fr(n * Lc)
    st = zk.DeviceBuffer.from_numpy(pp, np.full(7 * Lc, 0xAB, np.uint8))
    hb = h.to_numpy().copy()
    arr = lambda s: (C.c_uint32 * len(s))(*s)
    call = lambda ids, status: pp.lib.zk_circom_h_checked_parties(pp.h, arr(ids), len(ids), bufs[0].ptr, bufs[1].ptr,
                                                                  bufs[2].ptr, 3, None, SEED, h.ptr, status, None, None, None)
    for what, want, rc in (("a short list", PROTOCOL, call([0, 1, 2, 3, 4, 5], st.ptr)),
                           ("a list of 2l", PROTOCOL, call([0, 1, 2, 3], st.ptr)),
                           ("an unsorted list", BAD_INPUT, call([0, 1, 3, 2, 4, 5, 6], st.ptr)),
                           ("an id >= n", BAD_INPUT, call([0, 1, 2, 3, 4, 5, 8], st.ptr)),
                           ("more than n parties", BAD_INPUT, call(list(range(n + 1)), st.ptr)),
                           ("a null status", BAD_INPUT, call([0, 1, 2, 3, 4, 5, 6], None)),
                           ("a null status, all parties", BAD_INPUT, call(list(range(n)), None))):
        assert rc == want, what
        assert np.array_equal(h.to_numpy(), hb) and (st.to_numpy(np.uint8) == 0xAB).all(), what
    with pytest.raises(ValueError):
        api.circom_h(pp, bufs, None, SEED, check=False, log2_m=3, parties=list(range(n - 1)))
    # the context is still usable
    want, _ = _h(pp, rows, None, Lc, False)
    got, rep = _h_list(pp, rows, None, Lc, _without(pp, 3))
    assert np.array_equal(got, want) and _item_state(rep, Lc)[:6] == [(0, 0)] * 6 and _unchecked_row(pp, rep, Lc)
