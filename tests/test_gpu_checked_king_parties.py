"""GPU tests (through the C ABI) for the checked king rounds with a party list: zk_fft2_king_checked_parties,
zk_d_fft_checked_parties and zk_d_ifft_checked_parties repair the word the king receives from the listed parties
(zk_pss_repair_parties, dimension 2l, cap = (nparties - 2l) / 2) and then run the unchecked king with the same list.
  honest input         bit for bit the unchecked composition on the compact rows under the same seed: zk_fft1 with
                       batch = nparties, the mask rows, zk_fft2_king with the list; every status 0
  a known liar left out  the honest output and summary [Lc, 0, 0, 0...]: no chunk reached the decoder
  a liar beside an absent party   named by id, the output is the honest one
  more than cap liars  every chunk fails; the shares go to the king as received
The unchecked king takes a list only with more than 4l - 2 shares (unpack_missing_shares, pss.rs:183-186): with cap-many
parties absent that composition exists at l = 1 only; from l = 2 on zk_fft2_king answers ZK_ERR_PROTOCOL, and the checked
calls must answer the same before they write anything.
m / l = 512 chunks are two king workgroups and two workgroups of the scan (four at l = 8); m / l = 4 is one partial
workgroup: the sizes of test_gpu_checked_king.py."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk

from gpu_util import ctx, opp

CONFIGS = [("bn254", 1), ("bn254", 2), ("bn254", 4), ("bn254", 8), ("bls12_381", 2), ("bls12_377", 2)]
IDS = ["%s_l%d" % c for c in CONFIGS]
SIZES = [512, 4]
G = 5                      # the coset shift of the d_ifft cases
BAD_INPUT, PROTOCOL = 4, 2


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
    return zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(arr))


def _mask(pp, masked, inverse, rearrange, Lc, seed):
    if not masked:
        return zk.FftMask.zero()
    return zk.FftMask.sample(pp, rearrange, G if inverse else None, inverse, _log_m(pp, Lc), seed)


def _checked(pp, rows, S, mask, inverse, rearrange, Lc, seed):
    """zk_d_fft_checked_parties / zk_d_ifft_checked_parties out of place on a fresh copy of `rows` [n][Lc] -> (output, report)"""
    out = pp.alloc_fr(pp.n * Lc)
    fn = zk.d_ifft if inverse else zk.d_fft
    kw = {"g": G} if inverse else {}
    r = fn(pp, _dev(pp, rows), mask, rearrange, _log_m(pp, Lc), seed=seed, out=out, check=True, parties=S, **kw)
    assert r.out is out and r.parties == list(S)
    return out.to_numpy().reshape(pp.n, Lc, 4), r


def _received(pp, rows, S, mask, inverse, Lc):
    """the word the king receives from the listed parties, [|S|][Lc] on the device, by the unchecked calls: zk_fft1 with
    batch = |S| on the compact rows and the mask rows through add_d; for the masked inverse zk_vec_scale by 1 / m and
    zk_vec_add between the two.  -> (buffer, whether the king still has to scale by 1 / m)"""
    S = list(S)
    log_m, cnt = _log_m(pp, Lc), len(S) * Lc
    buf = _dev(pp, rows[S])
    mrows = None if mask.in_mask is None else _dev(pp, mask.in_mask.to_numpy().reshape(pp.n, Lc, 4)[S])
    if inverse and mrows is not None:
        pp._check(pp.lib.zk_fft1(pp.h, buf.ptr, log_m, 1, len(S), None, None))
        minv = pp.fr.encode_one(pow(1 << log_m, -1, opp(pp.curve, pp.l).p))
        pp._check(pp.lib.zk_vec_scale(pp.h, buf.ptr, minv.ctypes.data, cnt, None))
        pp._check(pp.lib.zk_vec_add(pp.h, buf.ptr, mrows.ptr, cnt, None))
        return buf, False
    pp._check(pp.lib.zk_fft1(pp.h, buf.ptr, log_m, int(inverse), len(S), None if mrows is None else mrows.ptr, None))
    return buf, bool(inverse)


def _unchecked(pp, rows, S, mask, inverse, rearrange, Lc, seed):
    """the unchecked list composition on `rows` -> output [n][Lc][4]"""
    buf, scale = _received(pp, rows, S, mask, inverse, Lc)
    out = zk.fft2_king(pp, buf, _log_m(pp, Lc), inverse=bool(inverse), g=G if inverse else None, scale_size_inv=scale,
                       rearrange=bool(rearrange), seed=seed, out_mask=mask.out_mask, parties=list(S))
    return out.to_numpy().reshape(pp.n, Lc, 4)


def _all(r, status, errpos, Lc):
    return (r.status_host() == status).all() and (r.errpos_host() == errpos).all() and len(r.status_host()) == Lc


def _summary(pp, Lc, status, parties=()):
    s = [0] * (3 + pp.n)
    s[status] = Lc
    for p in parties:
        s[3 + p] = Lc
    return s


def _lists(pp, seed):
    """one party absent (the first, a middle one or the last) and cap-many absent, cap = (n - 2l) / 2 = l"""
    n, l = pp.n, pp.l
    rnd = random.Random(seed)
    one = [q for q in range(n) if q != rnd.choice([0, n // 2, n - 1])]
    cap = (n - 2 * l) // 2
    many = sorted(rnd.sample(range(n), n - cap))
    return [one, many]


def _king_takes(pp, S):
    """zk_fft2_king's own condition on a list (pss.rs:183-186)"""
    return len(S) == pp.n or len(S) > 4 * pp.l - 2


def _liars(pp, rows, parties, seed):
    cur = rows.copy()
    for p in parties:
        cur[p] = _raw(np.random.default_rng(seed + p), rows.shape[1])
    return cur


# ---------------------------------------------------------------- honest input
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_honest_transforms_equal_the_unchecked_list_composition(curve, l, Lc):
    pp = ctx(curve, l)
    rows = _honest(pp, Lc, 400 + l)
    for S in _lists(pp, 7 * l + Lc):
        assert len(S) > 2 * l
        for inverse in (0, 1):
            for masked in (False, True):
                for rearrange in (0, 1):
                    mask = _mask(pp, masked, inverse, rearrange, Lc, 410 + l)
                    what = (curve, l, Lc, S, inverse, masked, rearrange)
                    if not _king_takes(pp, S):
                        # the unchecked composition refuses this list, and so does the checked call: same code
                        codes = []
                        for fn in (_unchecked, _checked):
                            with pytest.raises(zk.ZkError) as e:
                                fn(pp, rows, S, mask, inverse, rearrange, Lc, 420)
                            codes.append(e.value.code)
                        assert codes == [PROTOCOL, PROTOCOL], what
                        continue
                    want = _unchecked(pp, rows, S, mask, inverse, rearrange, Lc, 420)
                    got, r = _checked(pp, rows, S, mask, inverse, rearrange, Lc, 420)
                    assert np.array_equal(got, want), what
                    assert _all(r, 0, 0, Lc) and r.summary == _summary(pp, Lc, 0), what


@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_all_parties_listed_equals_the_checked_call(curve, l):
    pp = ctx(curve, l)
    Lc = 4
    rows = _liars(pp, _honest(pp, Lc, 430 + l), [pp.n - 1], 431)
    mask = _mask(pp, True, 1, 1, Lc, 432)
    want = pp.alloc_fr(pp.n * Lc)
    ref = zk.d_ifft(pp, _dev(pp, rows), mask, True, _log_m(pp, Lc), g=G, seed=433, out=want, check=True)
    got, r = _checked(pp, rows, list(range(pp.n)), mask, 1, 1, Lc, 433)
    assert np.array_equal(got, want.to_numpy().reshape(got.shape))
    assert list(r.status_host()) == list(ref.status_host()) == [1] * Lc
    assert list(r.errpos_host()) == list(ref.errpos_host()) and r.summary == ref.summary


# ---------------------------------------------------------------- a lying party, named and then left out
@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_a_named_liar_left_out_gives_the_honest_output_and_nothing_reaches_the_decoder(curve, l, Lc):
    pp = ctx(curve, l)
    n = pp.n
    rows = _honest(pp, Lc, 440 + l)
    for i, bad in enumerate([0, n // 2, n - 1]):
        cur = _liars(pp, rows, [bad], 450)
        for inverse in (0, 1):
            rearrange = (i + inverse) % 2
            mask = _mask(pp, True, inverse, rearrange, Lc, 460 + 2 * i + inverse)
            # precondition (existing behaviour): with all parties listed the checked call names the liar
            out = pp.alloc_fr(n * Lc)
            fn, kw = (zk.d_ifft, {"g": G}) if inverse else (zk.d_fft, {})
            r = fn(pp, _dev(pp, cur), mask, rearrange, _log_m(pp, Lc), seed=470, out=out, check=True, **kw)
            assert _all(r, 1, 1 << bad, Lc) and r.summary == _summary(pp, Lc, 1, [bad])
            honest = out.to_numpy().reshape(n, Lc, 4).copy()
            named = [q for q in range(n) if r.summary[3 + q]]
            assert named == [bad]
            S = [q for q in range(n) if q not in named]
            got, r = _checked(pp, cur, S, mask, inverse, rearrange, Lc, 470)
            what = (curve, l, Lc, bad, inverse)
            assert np.array_equal(got, honest), what
            assert _all(r, 0, 0, Lc) and r.summary == [Lc, 0, 0] + [0] * n, what


@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", [c for c in CONFIGS if c[1] >= 2], ids=[i for c, i in zip(CONFIGS, IDS) if c[1] >= 2])
def test_a_liar_beside_an_absent_party_is_named_by_id(curve, l, Lc):
    """n - 1 listed parties correct (n - 1 - 2l) / 2 >= 1 wrong shares from l = 2 on (at l = 1 the cap is 0)"""
    pp = ctx(curve, l)
    n = pp.n
    rows = _honest(pp, Lc, 480 + l)
    for absent, bad, inverse in ((0, 1, 0), (n // 2, n - 1, 1), (n - 1, 0, 0), (1, 2, 1)):
        cur = _liars(pp, rows, [bad], 490)
        cur[absent] = 0                                    # never read
        S = [q for q in range(n) if q != absent]
        mask = _mask(pp, True, inverse, 1, Lc, 500 + inverse)
        honest = _unchecked(pp, rows, S, mask, inverse, 1, Lc, 510)
        got, r = _checked(pp, cur, S, mask, inverse, 1, Lc, 510)
        what = (curve, l, Lc, absent, bad, inverse)
        assert np.array_equal(got, honest), what
        assert _all(r, 1, 1 << bad, Lc) and r.summary == _summary(pp, Lc, 1, [bad]), what


@pytest.mark.parametrize("Lc", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_more_than_cap_liars_fail_every_chunk_and_reach_the_king_as_received(curve, l, Lc):
    """a random word lands within cap of a codeword with probability about n^cap / r: no case is left out"""
    pp = ctx(curve, l)
    n = pp.n
    rows = _honest(pp, Lc, 520 + l)
    S = [q for q in range(n) if q != n // 2]
    cap = (len(S) - 2 * l) // 2
    cur = _liars(pp, rows, random.Random(20 + l).sample(S, cap + 1), 530)
    for inverse, masked, rearrange in ((0, True, 0), (1, False, 1), (1, True, 0)):
        mask = _mask(pp, masked, inverse, rearrange, Lc, 540 + inverse)
        got, r = _checked(pp, cur, S, mask, inverse, rearrange, Lc, 550)
        what = (curve, l, Lc, inverse, masked)
        assert _all(r, 2, 0, Lc) and r.summary == _summary(pp, Lc, 2), what
        assert np.array_equal(got, _unchecked(pp, cur, S, mask, inverse, rearrange, Lc, 550)), what


# ---------------------------------------------------------------- zk_fft2_king_checked_parties alone
@pytest.mark.parametrize("curve,l", [c for c in CONFIGS if c[1] >= 2], ids=[i for c, i in zip(CONFIGS, IDS) if c[1] >= 2])
def test_the_checked_king_with_a_list_repairs_in_place(curve, l):
    pp = ctx(curve, l)
    n, Lc = pp.n, 512
    log_m = _log_m(pp, Lc)
    absent = n // 2
    S = [q for q in range(n) if q != absent]
    buf = _dev(pp, _honest(pp, Lc, 560 + l)[S])
    pp._check(pp.lib.zk_fft1(pp.h, buf.ptr, log_m, 0, len(S), None, None))
    honest = buf.to_numpy().reshape(len(S), Lc, 4).copy()
    rng = np.random.default_rng(570 + l)
    cap = (len(S) - 2 * l) // 2
    place = {0: [S[0]], 255: [S[-1]], 256: [absent + 1], Lc - 1: [S[1]],                  # single errors, named by id
             100: sorted(random.Random(l).sample(S, cap)),                                # cap errors: corrected
             300: sorted(random.Random(l + 1).sample(S, cap + 1))}                        # cap + 1: failed
    recv = honest.copy()
    for c, parties in place.items():
        for p in parties:
            recv[S.index(p), c] = _raw(rng)
    want_status, want_err = np.zeros(Lc, np.uint8), np.zeros(Lc, np.uint32)
    for c, parties in place.items():
        want_status[c] = 2 if c == 300 else 1
        want_err[c] = 0 if c == 300 else sum(1 << p for p in parties)
    in_d = _dev(pp, recv)
    r = zk.fft2_king_checked_parties(pp, in_d, S, log_m, rearrange=True, seed=580)
    assert np.array_equal(r.status_host(), want_status) and np.array_equal(r.errpos_host(), want_err)
    want_sum = [Lc - 6, 5, 1] + [sum(1 for c, ps in place.items() if c != 300 and p in ps) for p in range(n)]
    assert r.summary == want_sum and r.parties == S
    fixed = honest.copy()
    fixed[:, 300] = recv[:, 300]
    assert np.array_equal(in_d.to_numpy().reshape(len(S), Lc, 4), fixed)
    want = zk.fft2_king(pp, _dev(pp, fixed), log_m, rearrange=True, seed=580, parties=S)
    assert np.array_equal(r.out.to_numpy(), want.to_numpy())


def test_refusals_and_the_context_stays_usable():
    pp = ctx("bn254", 2)
    n, l, Lc = pp.n, pp.l, 4
    log_m = _log_m(pp, Lc)
    rows = _honest(pp, Lc, 590)
    S = list(range(n - 1))
    ids = (C.c_uint32 * len(S))(*S)
    in_d, out, st = _dev(pp, rows[S]), pp.alloc_fr(n * Lc), zk.DeviceBuffer(pp, Lc)
    king = pp.lib.zk_fft2_king_checked_parties
    # in place
    assert king(pp.h, in_d.ptr, ids, len(S), log_m, 0, None, 0, 0, 1, in_d.ptr, None, st.ptr, None, None, None) == BAD_INPUT
    # nparties <= 2l: too few shares to check anything
    few = (C.c_uint32 * (2 * l))(*range(2 * l))
    assert king(pp.h, in_d.ptr, few, 2 * l, log_m, 0, None, 0, 0, 1, out.ptr, None, st.ptr, None, None, None) == PROTOCOL
    full = _dev(pp, rows)
    dfft, difft = pp.lib.zk_d_fft_checked_parties, pp.lib.zk_d_ifft_checked_parties
    assert dfft(pp.h, full.ptr, few, 2 * l, None, None, 0, log_m, 1, out.ptr, st.ptr, None, None, None) == PROTOCOL
    assert difft(pp.h, full.ptr, few, 2 * l, None, None, 0, log_m, None, 1, out.ptr, st.ptr, None, None, None) == PROTOCOL
    for bad in ([0, 1, 2, 2, 4, 5, 6], [0, 1, 2, 4, 3, 5, 6], [0, 1, 2, 4, 5, 6, 8]):
        arr = (C.c_uint32 * len(bad))(*bad)
        assert dfft(pp.h, full.ptr, arr, len(bad), None, None, 0, log_m, 1, out.ptr, st.ptr, None, None, None) == BAD_INPUT
        assert king(pp.h, in_d.ptr, arr, len(bad), log_m, 0, None, 0, 0, 1, out.ptr, None, st.ptr, None, None, None) == BAD_INPUT
    for count in (0, -1, n + 1):
        assert dfft(pp.h, full.ptr, None, count, None, None, 0, log_m, 1, out.ptr, st.ptr, None, None, None) == BAD_INPUT
    assert dfft(pp.h, full.ptr, ids, len(S), None, None, 0, log_m, 1, out.ptr, None, None, None, None) == BAD_INPUT
    with pytest.raises(zk.ZkError) as e:
        zk.d_fft(pp, full, zk.FftMask.zero(), False, log_m, check=True, parties=list(range(2 * l)))
    assert e.value.code == PROTOCOL
    assert np.array_equal(in_d.to_numpy().reshape(len(S), Lc, 4), rows[S])
    assert np.array_equal(full.to_numpy().reshape(n, Lc, 4), rows)
    # NULL errpos and summary; the context is still usable
    pp._check(king(pp.h, in_d.ptr, ids, len(S), log_m, 0, None, 0, 0, 1, out.ptr, None, st.ptr, None, None, None))
    assert not st.to_numpy(np.uint8)[:Lc].any()
    r = zk.fft2_king_checked_parties(pp, in_d, S, log_m, seed=1)
    assert np.array_equal(r.out.to_numpy(), out.to_numpy()) and r.summary == _summary(pp, Lc, 0)
    want = zk.fft2_king(pp, in_d, log_m, seed=1, parties=S)
    assert np.array_equal(want.to_numpy(), out.to_numpy())
