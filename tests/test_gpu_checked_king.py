"""GPU tests (through the C ABI) for the checked king rounds: zk_fft2_king_checked, zk_d_fft_checked, zk_d_ifft_checked and
zk_deg_red_checked repair the word the king receives (zk_pss_repair) and then run the unchecked king on it.
  honest input      the output is bit for bit the unchecked call's under the same seed (and the oracle's), every status 0
  up to l liars     d_fft / d_ifft give the honest output, the liars are named in errpos and counted in the summary
  l + 1 liars       every chunk fails; the shares go to the king as received
  deg_red           dimension 4l - 1, cap 0: detection only, nothing is rewritten
m / l = 512 chunks are two king workgroups (the wrapped chunk Lc - 1 is workgroup 0's) and two workgroups of the scan (four at
l = 8); m / l = 4 is one partial workgroup."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from oracle import dist as od
from oracle.field import Domain, bitrev_permute
from oracle.params import CURVES
from oracle.prng import rand_vec

from gpu_util import ctx, opp, up_parties, down_parties

CONFIGS = [("bn254", 1), ("bn254", 2), ("bn254", 4), ("bn254", 8), ("bls12_381", 2), ("bls12_377", 2)]
IDS = ["%s_l%d" % c for c in CONFIGS]
SIZES = [512, 4]
G = 5                      # the coset shift of the d_ifft cases


def _raw(rng, *shape):
    """random field elements as limbs: anything below 2^252 is one, in Montgomery form, for all three scalar fields"""
    a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


def _log_m(pp, Lc):
    return (Lc * pp.l).bit_length() - 1


def _honest(pp, Lc, seed):
    """packed shares [n][Lc][4] of random secrets"""
    sec = zk.DeviceBuffer.from_numpy(pp, _raw(np.random.default_rng(seed), Lc * pp.l))
    return pp.pack(sec, Lc, seed=seed).to_numpy().reshape(pp.n, Lc, 4).copy()


def _dev(pp, arr):
    return zk.DeviceBuffer.from_numpy(pp, arr)


def _transform(pp, rows, mask, inverse, rearrange, Lc, seed, check):
    """d_fft / d_ifft out of place on a fresh copy of `rows` -> (output array, report or None)"""
    out = pp.alloc_fr(pp.n * Lc)
    fn = zk.d_ifft if inverse else zk.d_fft
    kw = {"g": G} if inverse else {}
    r = fn(pp, _dev(pp, rows), mask, rearrange, _log_m(pp, Lc), seed=seed, out=out, check=check, **kw)
    return out.to_numpy().reshape(pp.n, Lc, 4), (r if check else None)


def _mask(pp, masked, inverse, rearrange, Lc, seed):
    if not masked:
        return zk.FftMask.zero()
    return zk.FftMask.sample(pp, rearrange, G if inverse else None, inverse, _log_m(pp, Lc), seed)


def _all(r, status, errpos, Lc):
    return (r.status_host() == status).all() and (r.errpos_host() == errpos).all() and len(r.status_host()) == Lc


def _summary(pp, Lc, status, parties=()):
    s = [0] * (3 + pp.n)
    s[status] = Lc
    for p in parties:
        s[3 + p] = Lc
    return s


# ---------------------------------------------------------------- honest input
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_honest_transforms_equal_the_unchecked_calls(curve, l, Lc):
    pp = ctx(curve, l)
    rows = _honest(pp, Lc, 100 + l)
    for inverse in (0, 1):
        for masked in (False, True):
            for rearrange in (0, 1):
                mask = _mask(pp, masked, inverse, rearrange, Lc, 110 + l)
                want, _ = _transform(pp, rows, mask, inverse, rearrange, Lc, 120, False)
                got, r = _transform(pp, rows, mask, inverse, rearrange, Lc, 120, True)
                what = (curve, l, Lc, inverse, masked, rearrange)
                assert np.array_equal(got, want), what
                assert _all(r, 0, 0, Lc) and r.summary == _summary(pp, Lc, 0), what


def _deal(x, o, seed):
    y = list(x)
    bitrev_permute(y)
    return od.transpose(od.stride_pack(y, o, seed))


@pytest.mark.parametrize("inverse", [0, 1])
def test_honest_transforms_equal_the_oracle(inverse):
    curve, l, m = "bn254", 2, 64
    pp, o = ctx(curve, l), opp(curve, l)
    dom = Domain(CURVES[curve], m)
    g = Domain(CURVES[curve], 2 * m).element(1)
    shares = _deal(rand_vec(130, m, o.p), o, 131)
    if inverse:
        masks = od.FftMask.sample(True, g, dom.group_gen_inv, m, o, 132)
        want = od.d_ifft(shares, masks, True, dom, g, o, seed=133)
    else:
        masks = od.FftMask.sample(False, 1, dom.group_gen, m, o, 132)
        want = od.d_fft(shares, masks, False, dom, o, seed=133)
    buf = up_parties(pp, shares)
    fm = zk.FftMask(up_parties(pp, [mk.in_mask for mk in masks]), up_parties(pp, [mk.out_mask for mk in masks]))
    if inverse:
        r = zk.d_ifft(pp, buf, fm, True, 6, g=g, seed=133, check=True)
    else:
        r = zk.d_fft(pp, buf, fm, False, 6, seed=133, check=True)
    assert r.out is buf and down_parties(pp, buf, pp.n, m // l) == want
    assert _all(r, 0, 0, m // l) and r.summary == _summary(pp, m // l, 0)


# ---------------------------------------------------------------- lying parties
def _liars(pp, rows, parties, seed):
    cur = rows.copy()
    for p in parties:
        cur[p] = _raw(np.random.default_rng(seed + p), rows.shape[1])
    return cur


@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_one_lying_party_is_named_and_the_output_is_the_honest_one(curve, l, Lc):
    pp = ctx(curve, l)
    rows = _honest(pp, Lc, 140 + l)
    liars = [0, pp.n // 2, pp.n - 1]                  # the first, a middle and the last party: three ids at every l (n >= 4)
    assert len(set(liars)) == 3 and 0 < liars[1] < pp.n - 1
    for i, bad in enumerate(liars):
        cur = _liars(pp, rows, [bad], 170)
        for inverse in (0, 1):
            rearrange = (i + inverse) % 2
            mask = _mask(pp, True, inverse, rearrange, Lc, 150 + 2 * i + inverse)
            honest, _ = _transform(pp, rows, mask, inverse, rearrange, Lc, 160, False)
            got, r = _transform(pp, cur, mask, inverse, rearrange, Lc, 160, True)
            what = (curve, l, Lc, bad, inverse)
            assert np.array_equal(got, honest), what
            assert _all(r, 1, 1 << bad, Lc) and r.summary == _summary(pp, Lc, 1, [bad]), what
            unchecked, _ = _transform(pp, cur, mask, inverse, rearrange, Lc, 160, False)
            assert not np.array_equal(unchecked, honest), what          # the test sees the defect the check removes


@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", [c for c in CONFIGS if c[1] >= 2], ids=[i for c, i in zip(CONFIGS, IDS) if c[1] >= 2])
def test_l_lying_parties_are_still_corrected(curve, l, Lc):
    pp = ctx(curve, l)
    rows = _honest(pp, Lc, 180 + l)
    bad = sorted(random.Random(l).sample(range(pp.n), l))
    for inverse in (0, 1):
        mask = _mask(pp, bool(inverse), inverse, 1, Lc, 190)
        honest, _ = _transform(pp, rows, mask, inverse, 1, Lc, 200, False)
        got, r = _transform(pp, _liars(pp, rows, bad, 210), mask, inverse, 1, Lc, 200, True)
        assert np.array_equal(got, honest), (curve, l, Lc, inverse)
        assert _all(r, 1, sum(1 << p for p in bad), Lc) and r.summary == _summary(pp, Lc, 1, bad), (curve, l, Lc, inverse)


@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_l_plus_one_lying_parties_fail_every_chunk_and_reach_the_king_as_received(curve, l, Lc):
    """a random word lands within cap of a codeword with probability about n^cap / r: no case is left out"""
    pp = ctx(curve, l)
    log_m = _log_m(pp, Lc)
    rows = _honest(pp, Lc, 220 + l)
    cur = _liars(pp, rows, random.Random(10 + l).sample(range(pp.n), l + 1), 230)
    # d_fft with masks: the received matrix is fft1(x) + in_mask
    mask = _mask(pp, True, 0, 0, Lc, 240)
    got, r = _transform(pp, cur, mask, 0, 0, Lc, 250, True)
    assert _all(r, 2, 0, Lc) and r.summary == _summary(pp, Lc, 2), (curve, l, Lc)
    recv = _dev(pp, cur)
    pp._check(pp.lib.zk_fft1(pp.h, recv.ptr, log_m, 0, pp.n, mask.in_mask.ptr, None))
    want = zk.fft2_king(pp, recv, log_m, seed=250, out_mask=mask.out_mask)
    assert np.array_equal(got, want.to_numpy().reshape(pp.n, Lc, 4)), (curve, l, Lc)
    # d_ifft without masks: the received matrix is fft1(x), the king scales by 1 / m
    got, r = _transform(pp, cur, zk.FftMask.zero(), 1, 1, Lc, 251, True)
    assert _all(r, 2, 0, Lc) and r.summary == _summary(pp, Lc, 2), (curve, l, Lc)
    recv = _dev(pp, cur)
    pp._check(pp.lib.zk_fft1(pp.h, recv.ptr, log_m, 1, pp.n, None, None))
    want = zk.fft2_king(pp, recv, log_m, inverse=True, g=G, scale_size_inv=True, rearrange=True, seed=251)
    assert np.array_equal(got, want.to_numpy().reshape(pp.n, Lc, 4)), (curve, l, Lc)
    # d_ifft with masks: as the unchecked call on the same input
    mask = _mask(pp, True, 1, 0, Lc, 241)
    got, r = _transform(pp, cur, mask, 1, 0, Lc, 252, True)
    want, _ = _transform(pp, cur, mask, 1, 0, Lc, 252, False)
    assert _all(r, 2, 0, Lc) and np.array_equal(got, want), (curve, l, Lc)


# ---------------------------------------------------------------- sparse errors through zk_fft2_king_checked
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_sparse_errors_through_the_checked_king(curve, l):
    pp = ctx(curve, l)
    n, Lc = pp.n, 512
    log_m = _log_m(pp, Lc)
    buf = _dev(pp, _honest(pp, Lc, 260 + l))
    pp._check(pp.lib.zk_fft1(pp.h, buf.ptr, log_m, 0, n, None, None))
    honest = buf.to_numpy().reshape(n, Lc, 4).copy()
    rng = np.random.default_rng(270 + l)
    place = {0: [1 % n], 1: [n - 1], 255: [0], 256: [n // 2], Lc - 1: [2 % n],       # single errors at different parties
             100: sorted(random.Random(l).sample(range(n), l)),                        # l errors: corrected
             300: sorted(random.Random(l + 1).sample(range(n), l + 1))}                # l + 1: failed
    recv = honest.copy()
    for c, parties in place.items():
        for p in parties:
            recv[p, c] = _raw(rng)
    want_status, want_err = np.zeros(Lc, np.uint8), np.zeros(Lc, np.uint32)
    for c, parties in place.items():
        want_status[c] = 2 if c == 300 else 1
        want_err[c] = 0 if c == 300 else sum(1 << p for p in parties)
    in_d = _dev(pp, recv)
    r = zk.fft2_king(pp, in_d, log_m, rearrange=True, seed=280, check=True)
    assert np.array_equal(r.status_host(), want_status) and np.array_equal(r.errpos_host(), want_err)
    want_sum = [Lc - 7, 6, 1] + [sum(1 for c, ps in place.items() if c != 300 and p in ps) for p in range(n)]
    assert r.summary == want_sum
    fixed = honest.copy()
    fixed[:, 300] = recv[:, 300]
    assert np.array_equal(in_d.to_numpy().reshape(n, Lc, 4), fixed)
    want = zk.fft2_king(pp, _dev(pp, fixed), log_m, rearrange=True, seed=280)
    assert np.array_equal(r.out.to_numpy(), want.to_numpy())


# ---------------------------------------------------------------- deg_red: detection only
def _products(pp, nch, seed):
    """x = a * b element by element for two packed sharings: words of degree 4l - 2, the dimension of deg_red"""
    a, b = _dev(pp, _honest(pp, nch, seed)), _dev(pp, _honest(pp, nch, seed + 1))
    zero = _dev(pp, np.zeros((pp.n * nch, 4), np.uint64))
    out = pp.alloc_fr(pp.n * nch)
    pp._check(pp.lib.zk_vec_mul_sub(pp.h, out.ptr, a.ptr, b.ptr, zero.ptr, pp.n * nch, None))
    return out.to_numpy().reshape(pp.n, nch, 4).copy()


@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_deg_red_checked_detects_and_never_rewrites(curve, l):
    pp = ctx(curve, l)
    n, nch = pp.n, 331
    x = _products(pp, nch, 290 + l)
    rng = np.random.default_rng(300 + l)
    for masked in (False, True):
        mask = zk.DegRedMask.sample(pp, nch, 310) if masked else zk.DegRedMask.zero()
        for name, dirty in (("honest", []), ("first", [0]), ("last", [330]), ("all", list(range(nch)))):
            cur = x.copy()
            for c in dirty:
                cur[int(rng.integers(n)), c] = _raw(rng)
            want = zk.deg_red(pp, _dev(pp, cur), mask, nch, seed=320)
            buf = _dev(pp, cur)
            r = zk.deg_red(pp, buf, mask, nch, seed=320, check=True)
            assert r.out is buf and np.array_equal(buf.to_numpy(), want.to_numpy()), (curve, l, masked, name)
            want_status = np.zeros(nch, np.uint8)
            want_status[dirty] = 2
            assert np.array_equal(r.status_host(), want_status) and not r.errpos_host().any(), (curve, l, masked, name)
            assert r.summary == [nch - len(dirty), 0, len(dirty)] + [0] * n, (curve, l, masked, name)


def test_deg_red_checked_equals_the_oracle():
    curve, l, nch = "bn254", 2, 5
    pp, o = ctx(curve, l), opp(curve, l)
    a = od.transpose(od.pack_vec(rand_vec(330, nch * l, o.p), o, 331))
    b = od.transpose(od.pack_vec(rand_vec(332, nch * l, o.p), o, 333))
    xs = [[u * v % o.p for u, v in zip(ra, rb)] for ra, rb in zip(a, b)]
    masks = od.DegRedMask.sample(o, 1, nch, 334)
    want = od.deg_red(xs, masks, o, seed=335)
    buf = up_parties(pp, xs)
    dm = zk.DegRedMask(up_parties(pp, [k.in_mask for k in masks]), up_parties(pp, [k.out_mask for k in masks]))
    r = zk.deg_red(pp, buf, dm, nch, seed=335, check=True)
    assert down_parties(pp, buf, pp.n, nch) == want
    assert _all(r, 0, 0, nch) and r.summary == [nch, 0, 0] + [0] * pp.n


# ---------------------------------------------------------------- error returns, two streams
def test_deg_red_checked_bad_input_leaves_x_unchanged():
    pp = ctx("bn254", 2)
    nch = 7
    x = _products(pp, nch, 336)
    mask = zk.DegRedMask.sample(pp, nch, 337)
    buf = _dev(pp, x)
    rc = pp.lib.zk_deg_red_checked(pp.h, buf.ptr, mask.in_mask.ptr, mask.out_mask.ptr, nch, 338, None, None, None, None)
    assert rc == 4 and np.array_equal(buf.to_numpy().reshape(pp.n, nch, 4), x)       # no mask was added
    assert pp.lib.zk_deg_red_checked(pp.h, None, mask.in_mask.ptr, None, nch, 338, None, None, None, None) == 4
    assert pp.lib.zk_deg_red_checked(pp.h, None, None, None, 0, 338, None, None, None, None) == 0
    # the context is still usable
    want = zk.deg_red(pp, _dev(pp, x), mask, nch, seed=338)
    r = zk.deg_red(pp, buf, mask, nch, seed=338, check=True)
    assert np.array_equal(buf.to_numpy(), want.to_numpy()) and r.summary == [nch, 0, 0] + [0] * pp.n


def test_a_party_list_is_bad_input_and_the_context_stays_usable():
    pp = ctx("bn254", 2)
    n, Lc = pp.n, 4
    log_m = _log_m(pp, Lc)
    rows = _honest(pp, Lc, 340)
    in_d, out = _dev(pp, rows), pp.alloc_fr(n * Lc)
    st, ids = zk.DeviceBuffer(pp, Lc), (C.c_uint32 * (n - 1))(*range(n - 1))
    for parties, count in ((ids, n - 1), (None, n - 1), (None, n + 1)):
        rc = pp.lib.zk_fft2_king_checked(pp.h, in_d.ptr, parties, count, log_m, 0, None, 0, 0, 1, out.ptr, None, st.ptr, None,
                                         None, None)
        assert rc == 4
    with pytest.raises(zk.ZkError) as e:
        zk.fft2_king(pp, in_d, log_m, parties=list(range(n - 1)), check=True)
    assert e.value.code == 4 and "unchecked" in e.value.msg
    assert np.array_equal(in_d.to_numpy().reshape(n, Lc, 4), rows)
    # NULL errpos and summary; then the wrappers
    pp._check(pp.lib.zk_fft2_king_checked(pp.h, in_d.ptr, None, n, log_m, 0, None, 0, 0, 1, out.ptr, None, st.ptr, None, None,
                                          None))
    assert not st.to_numpy(np.uint8)[:Lc].any()
    r = zk.fft2_king(pp, in_d, log_m, seed=1, check=True)
    assert np.array_equal(r.out.to_numpy(), out.to_numpy()) and r.summary == _summary(pp, Lc, 0)


def _streams(pp, count):
    """HIP streams from the runtime the library is linked against (its symbols resolve through the library's handle)"""
    create = pp.lib.hipStreamCreate
    create.argtypes, create.restype = [C.POINTER(C.c_void_p)], C.c_int
    out = []
    for _ in range(count):
        st = C.c_void_p()
        assert create(C.byref(st)) == 0
        out.append(st)
    return out


def test_checked_calls_on_two_streams_equal_the_serial_results():
    pp = ctx("bn254", 2)
    Lc = 512
    log_m = _log_m(pp, Lc)
    rows = [_liars(pp, _honest(pp, Lc, 350 + i), [3 + i], 360) for i in range(2)]
    masks = [zk.FftMask.sample(pp, True, G, True, log_m, 370 + i) for i in range(2)]
    xs = [_dev(pp, rows[i]) for i in range(2)]
    pp.sync()

    def run(i, stream):
        a = zk.d_ifft(pp, xs[i], masks[i], True, log_m, g=G, seed=380 + i, out=pp.alloc_fr(pp.n * Lc), stream=stream, check=True)
        b = zk.d_fft(pp, a.out, zk.FftMask.zero(), False, log_m, seed=390 + i, out=pp.alloc_fr(pp.n * Lc), stream=stream,
                     check=True)
        return a, b

    def snap(reports):
        return [(r.out.to_numpy().copy(), r.status_host().copy(), r.errpos_host().copy(), r.summary) for r in reports]

    serial = []
    for i in range(2):
        serial.append(snap(run(i, None)))
        pp.sync()
        assert serial[i][0][3] == _summary(pp, Lc, 1, [3 + i]) and serial[i][1][3] == _summary(pp, Lc, 0)
    streams = _streams(pp, 2)
    for rep in range(5):
        outs = [run(i, streams[i]) for i in range(2)]
        for st in streams:
            pp.sync(st)
        for i in range(2):
            for got, want in zip(snap(outs[i]), serial[i]):
                assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3], (rep, i)
    destroy = pp.lib.hipStreamDestroy
    destroy.argtypes, destroy.restype = [C.c_void_p], C.c_int
    for st in streams:
        assert destroy(st) == 0
