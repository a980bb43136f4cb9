"""GPU tests (through the C ABI) for zk_circom_h_checked: circom_h (ext_wit.rs:104-181) with each of its seven king words
repaired before the king reads it -- items 0..2 the d_ifft words of a, b, c, items 3..5 the d_fft words, item 6 the deg_red
word (dimension 4l - 1: detection only).
  honest input   h is bit for bit zk_circom_h's under the same seed and masks (and the oracle's), every status 0
  round 1        wrong rows in the QAP share vectors: h is the honest h, the parties are named per item
  round 2        a wrong row in an in-mask of the d_fft round: h is the h of the untampered masks, the party is named
  deg_red        a wrong row in its in-mask: status 2 everywhere, nothing rewritten, h is zk_circom_h's on the same masks
  l + 1 liars    item 0 fails in every chunk, h is zk_circom_h's on the same input
m / l = 512 chunks are two workgroups of the scan per item (four at l = 8), m / l = 4 is one partial workgroup.  Mask sets: all
twelve masks, none, and the in-masks of both rounds partly present (the kings then run item by item)."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import api
from zksaas_amd import groth16 as zg
from oracle import dist as od
from oracle import groth16 as og
from oracle.field import Domain
from oracle.params import BN254

from gpu_util import ctx, opp, up_parties, down_parties

CONFIGS = [("bn254", 1), ("bn254", 2), ("bn254", 4), ("bn254", 8), ("bls12_381", 2)]
IDS = ["%s_l%d" % c for c in CONFIGS]
SIZES = [512, 4]
MASK_SETS = ["all", "none", "partial"]
BAD_INPUT = 4
SEED = 77


def _raw(rng, *shape):
    """random field elements as limbs: anything below 2^252 is one, in Montgomery form, for the scalar fields used here"""
    a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


def _log_m(pp, Lc):
    return (Lc * pp.l).bit_length() - 1


_qap, _masks = {}, {}


def _honest(pp, Lc):
    """three matrices [n][Lc][4] of packed shares, computed once per shape and never changed: the callers copy"""
    key = (pp.curve, pp.l, Lc)
    if key not in _qap:
        rows = []
        for k in range(3):
            sec = zk.DeviceBuffer.from_numpy(pp, _raw(np.random.default_rng(500 + k), Lc * pp.l))
            rows.append(pp.pack(sec, Lc, seed=510 + k).to_numpy().reshape(pp.n, Lc, 4).copy())
        _qap[key] = rows
    return _qap[key]


def _dev(pp, arr):
    return zk.DeviceBuffer.from_numpy(pp, arr)


def _copy_masks(ct):
    mk = zg.Masks()
    C.memmove(C.byref(mk), C.byref(ct), C.sizeof(zg.Masks))
    return mk


def _mask_set(pp, Lc, which):
    """a zk_groth16_masks (or None) -- the dealt buffers are shared among the tests and never written"""
    if which == "none":
        return None
    key = (pp.curve, pp.l, Lc)
    if key not in _masks:
        _masks[key] = zg.ProofMasks(pp, _log_m(pp, Lc), 520)
    mk = _copy_masks(_masks[key].ct)
    if which == "partial":
        for k in (1, 3, 4):                     # round 1: a and c masked; round 2: c only
            mk.fft_in[k] = None
    return mk


def _h(pp, rows, mk, Lc, check):
    bufs = [_dev(pp, r) for r in rows]
    out = api.circom_h(pp, bufs, mk, SEED, check=check, log2_m=_log_m(pp, Lc))
    if not check:
        return out.to_numpy(), None
    return out[0].to_numpy(), out[1]


def _item_state(rep, Lc):
    """per item: (status, errpos) when all chunks agree, else None"""
    st, ep = rep.status_host().reshape(7, Lc), rep.errpos_host().reshape(7, Lc)
    return [(int(st[i, 0]), int(ep[i, 0])) if (st[i] == st[i, 0]).all() and (ep[i] == ep[i, 0]).all() else None
            for i in range(7)]


def _summary(pp, Lc, status, parties=()):
    s = [0] * (3 + pp.n)
    s[status] = Lc
    for p in parties:
        s[3 + p] = Lc
    return s


def _liars(rows, parties, seed):
    cur = rows.copy()
    for p in parties:
        cur[p] = _raw(np.random.default_rng(seed + p), rows.shape[1])
    return cur


def _tampered_mask(pp, mk, name, k, p, seed, Lc):
    """the mask set with party p's row of one in-mask replaced -> (masks, the buffer that holds the row)"""
    ptr = getattr(mk, name)[k] if k is not None else getattr(mk, name)
    src = zk.DeviceBuffer.__new__(zk.DeviceBuffer)
    src.ctx, src.ptr, src.nbytes, src.owner = pp, ptr, pp.n * Lc * 32, False
    rows = src.to_numpy().reshape(pp.n, Lc, 4).copy()
    buf = _dev(pp, _liars(rows, [p], seed))
    out = _copy_masks(mk)
    if k is None:
        setattr(out, name, buf.ptr)
    else:
        getattr(out, name)[k] = buf.ptr
    return out, buf


# ---------------------------------------------------------------- honest input
@pytest.mark.parametrize("which", MASK_SETS)
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_honest_h_equals_the_unchecked_chain(curve, l, Lc, which):
    pp = ctx(curve, l)
    rows, mk = _honest(pp, Lc), _mask_set(pp, Lc, which)
    want, _ = _h(pp, rows, mk, Lc, False)
    got, rep = _h(pp, rows, mk, Lc, True)
    assert np.array_equal(got, want), (curve, l, Lc, which)
    assert _item_state(rep, Lc) == [(0, 0)] * 7, (curve, l, Lc, which)
    assert rep.summaries == [_summary(pp, Lc, 0)] * 7, (curve, l, Lc, which)
    # the report is optional but for the status
    bufs, h = [_dev(pp, r) for r in rows], pp.alloc_fr(pp.n * Lc)
    st = zk.DeviceBuffer.from_numpy(pp, np.full(7 * Lc, 0xAB, np.uint8))
    pp._check(pp.lib.zk_circom_h_checked(pp.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, _log_m(pp, Lc),
                                         None if mk is None else C.byref(mk), SEED, h.ptr, st.ptr, None, None, None))
    assert np.array_equal(h.to_numpy(), want) and not st.to_numpy(np.uint8).any(), (curve, l, Lc, which)


def test_honest_h_equals_the_oracle():  # ext_wit.rs:419-538 (a = b = [0..m), c = a*b), masked
    m, l = 64, 2
    pp, o = ctx("bn254", l), opp("bn254", l)
    P = BN254.r
    dom = Domain(BN254, m)
    a = list(range(m))
    c = [x * x % P for x in a]
    qs = og.QAP(0, 0, a, a, c, dom).pss(o, 3)
    w2m = Domain(BN254, 2 * m).element(1)
    fm = ([od.FftMask.sample(True, w2m, dom.group_gen_inv, m, o, 40 + k) for k in range(3)]
          + [od.FftMask.sample(False, 1, dom.group_gen, m, o, 50 + k) for k in range(3)])
    dm = od.DegRedMask.sample(o, 1, m // l, 60)
    want = og.circom_h(qs, fm, dm, o, dom, seed=4)
    bufs = [up_parties(pp, [qs[i][k] for i in range(o.n)]) for k in range(3)]
    keep = []
    mk = zg.Masks()
    for k in range(6):
        bi = up_parties(pp, [x.in_mask for x in fm[k]])
        bo = up_parties(pp, [x.out_mask for x in fm[k]])
        keep += [bi, bo]
        mk.fft_in[k], mk.fft_out[k] = bi.ptr, bo.ptr
    di, do = up_parties(pp, [x.in_mask for x in dm]), up_parties(pp, [x.out_mask for x in dm])
    mk.degred_in, mk.degred_out = di.ptr, do.ptr
    h, rep = api.circom_h(pp, bufs, mk, 4, check=True, log2_m=6)
    assert down_parties(pp, h, o.n, m // l) == want
    assert _item_state(rep, m // l) == [(0, 0)] * 7 and rep.summaries == [_summary(pp, m // l, 0)] * 7
    assert pp.download_fr(pp.unpack2(h, m // l)) == og.circom_ref(a, a, c, dom)


# ---------------------------------------------------------------- round 1: wrong QAP shares
@pytest.mark.parametrize("which", ["all", "partial"])
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_round_1_liars_are_named_and_h_is_the_honest_one(curve, l, Lc, which):
    pp = ctx(curve, l)
    rows, mk = _honest(pp, Lc), _mask_set(pp, Lc, which)
    honest, _ = _h(pp, rows, mk, Lc, False)
    p, q = pp.n - 1, 1
    cur = [_liars(rows[0], [p], 530), _liars(rows[1], [q], 540), rows[2]]
    got, rep = _h(pp, cur, mk, Lc, True)
    assert np.array_equal(got, honest), (curve, l, Lc, which)
    assert _item_state(rep, Lc) == [(1, 1 << p), (1, 1 << q)] + [(0, 0)] * 5, (curve, l, Lc, which)
    assert rep.summaries == [_summary(pp, Lc, 1, [p]), _summary(pp, Lc, 1, [q])] + [_summary(pp, Lc, 0)] * 5
    unchecked, _ = _h(pp, cur, mk, Lc, False)
    assert not np.array_equal(unchecked, honest), (curve, l, Lc, which)         # the input bites
    if l >= 2:                                    # l liars in one vector are still corrected
        bad = sorted(random.Random(l).sample(range(pp.n), l))
        got, rep = _h(pp, [rows[0], rows[1], _liars(rows[2], bad, 550)], mk, Lc, True)
        assert np.array_equal(got, honest), (curve, l, Lc, which)
        assert _item_state(rep, Lc) == [(0, 0)] * 2 + [(1, sum(1 << b for b in bad))] + [(0, 0)] * 4
        assert rep.summaries[2] == _summary(pp, Lc, 1, bad), (curve, l, Lc, which)


# ---------------------------------------------------------------- round 2: a wrong row of an in-mask
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_round_2_liar_in_an_in_mask_is_named(curve, l, Lc):
    """the king's output of round 1 is honest on one device, so the liar enters with the row it adds itself"""
    pp = ctx(curve, l)
    rows, mk = _honest(pp, Lc), _mask_set(pp, Lc, "all")
    honest, _ = _h(pp, rows, mk, Lc, False)
    for k, p in ((0, 0), (1, pp.n // 2), (2, pp.n - 1)):
        bad, keep = _tampered_mask(pp, mk, "fft_in", 3 + k, p, 560 + k, Lc)
        got, rep = _h(pp, rows, bad, Lc, True)
        assert np.array_equal(got, honest), (curve, l, Lc, k)
        want = [(0, 0)] * 7
        want[3 + k] = (1, 1 << p)
        assert _item_state(rep, Lc) == want, (curve, l, Lc, k)
        assert rep.summaries[3 + k] == _summary(pp, Lc, 1, [p]), (curve, l, Lc, k)
        del keep


# ---------------------------------------------------------------- deg_red: detection only
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_deg_red_word_is_detection_only(curve, l, Lc):
    pp = ctx(curve, l)
    rows, mk = _honest(pp, Lc), _mask_set(pp, Lc, "all")
    p = pp.n // 2
    bad, keep = _tampered_mask(pp, mk, "degred_in", None, p, 570, Lc)
    want, _ = _h(pp, rows, bad, Lc, False)
    got, rep = _h(pp, rows, bad, Lc, True)
    assert np.array_equal(got, want), (curve, l, Lc)
    assert _item_state(rep, Lc) == [(0, 0)] * 6 + [(2, 0)], (curve, l, Lc)
    assert rep.summaries[6] == _summary(pp, Lc, 2) and rep.summaries[:6] == [_summary(pp, Lc, 0)] * 6, (curve, l, Lc)
    del keep


# ---------------------------------------------------------------- l + 1 liars: failed chunks reach the king as received
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_l_plus_one_liars_fail_every_chunk(curve, l, Lc):
    pp = ctx(curve, l)
    rows = _honest(pp, Lc)
    for which in ("all", "none"):
        mk = _mask_set(pp, Lc, which)
        cur = [_liars(rows[0], random.Random(20 + l).sample(range(pp.n), l + 1), 580), rows[1], rows[2]]
        want, _ = _h(pp, cur, mk, Lc, False)
        got, rep = _h(pp, cur, mk, Lc, True)
        assert np.array_equal(got, want), (curve, l, Lc, which)
        assert _item_state(rep, Lc)[:3] == [(2, 0), (0, 0), (0, 0)], (curve, l, Lc, which)
        assert rep.summaries[0] == _summary(pp, Lc, 2), (curve, l, Lc, which)


# ---------------------------------------------------------------- refusals
def test_refusals():
    pp = ctx("bn254", 2)
    Lc = 4
    rows = _honest(pp, Lc)
    bufs, h = [_dev(pp, r) for r in rows], pp.alloc_fr(pp.n * Lc)
    st = zk.DeviceBuffer.from_numpy(pp, np.full(7 * Lc, 0xAB, np.uint8))
    hb = h.to_numpy().copy()
    a, b, c = (x.ptr for x in bufs)
    call = lambda qa, qb, qc, log_m, out, status: pp.lib.zk_circom_h_checked(pp.h, qa, qb, qc, log_m, None, SEED, out, status,
                                                                             None, None, None)
    for what, rc in (("m < l", call(a, b, c, 0, h.ptr, st.ptr)), ("domain too large", call(a, b, c, 28, h.ptr, st.ptr)),
                     ("null a", call(None, b, c, 3, h.ptr, st.ptr)), ("null b", call(a, None, c, 3, h.ptr, st.ptr)),
                     ("null c", call(a, b, None, 3, h.ptr, st.ptr)), ("null h", call(a, b, c, 3, None, st.ptr)),
                     ("null status", call(a, b, c, 3, h.ptr, None))):
        assert rc == BAD_INPUT, what
        assert np.array_equal(h.to_numpy(), hb) and (st.to_numpy(np.uint8) == 0xAB).all(), what
    # the first six are zk_circom_h's own
    ucall = lambda qa, qb, qc, log_m, out: pp.lib.zk_circom_h(pp.h, qa, qb, qc, log_m, None, SEED, out, None)
    assert [ucall(a, b, c, 0, h.ptr), ucall(a, b, c, 28, h.ptr), ucall(None, b, c, 3, h.ptr), ucall(a, None, c, 3, h.ptr),
            ucall(a, b, None, 3, h.ptr), ucall(a, b, c, 3, None)] == [BAD_INPUT] * 6
    # the context is still usable
    want, _ = _h(pp, rows, None, Lc, False)
    got, rep = _h(pp, rows, None, Lc, True)
    assert np.array_equal(got, want) and _item_state(rep, Lc) == [(0, 0)] * 7
