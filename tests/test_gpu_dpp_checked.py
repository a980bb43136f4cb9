"""GPU tests (through the C ABI) for zk_d_pp_checked: the king of d_pp (dpp/mod.rs:37-52) receives num ++ den per party,
packed shares of degree < 2l; both words are repaired (zk_pss_repair_parties, dimension 2l) before the unchecked king runs.
  honest input      bit for bit zk_d_pp's output under the same seed, both summaries clean
  one liar          in num only, in den only, in both: named in the right half of status / errpos / summary, honest output
  l + 1 liars in den   that half fails; the call returns what zk_d_pp returns on the same received shares
  a party list      one party absent plus one liar, against oracle.dist.d_pp on the honest shares
len = 300 is more than one workgroup of the scan (and of the finish kernel), len = 4 one partial workgroup.  Secrets are
random and nonzero, so every reconstructed denominator is nonzero: checked on the host before the calls."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from oracle import dist as od
from oracle.prng import rand_vec

from gpu_util import ctx, opp, up_parties, down_parties

CONFIGS = [("bn254", 2), ("bn254", 8), ("bls12_381", 2)]
IDS = ["%s_l%d" % c for c in CONFIGS]
SIZES = [4, 300]


def _raw(rng, *shape):
    """random field elements as limbs: anything below 2^252 is one, in Montgomery form, for all three scalar fields"""
    a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


def _dev(pp, arr):
    return zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(arr))


def _honest(pp, length, seed):
    """(num, den) packed shares [n][length][4] of random nonzero secrets"""
    out = []
    for s in (seed, seed + 1):
        sec = _raw(np.random.default_rng(s), length * pp.l)
        assert sec.any(axis=-1).all()                     # Montgomery limbs of zero are zero: no secret is zero
        out.append(pp.pack(_dev(pp, sec), length, seed=s).to_numpy().reshape(pp.n, length, 4).copy())
    return out


def _liars(rows, parties, seed):
    cur = rows.copy()
    for p in parties:
        cur[p] = _raw(np.random.default_rng(seed + p), rows.shape[1])
    return cur


def _halves(r, length):
    st, err = r.status_host(), r.errpos_host()
    assert len(st) == len(err) == 2 * length
    return (st[:length], err[:length]), (st[length:], err[length:])


def _summary(pp, length, status, parties=()):
    s = [0] * (3 + pp.n)
    s[status] = length
    for p in parties:
        s[3 + p] = length
    return s


@pytest.mark.parametrize("length", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_honest_input_and_single_liars(curve, l, length):
    pp = ctx(curve, l)
    n = pp.n
    num, den = _honest(pp, length, 600 + l)
    mask = zk.DegRedMask.sample(pp, length, 610 + l)
    want = zk.d_pp(pp, _dev(pp, num), _dev(pp, den), mask, length, seed=620).to_numpy().copy()
    r = zk.d_pp(pp, _dev(pp, num), _dev(pp, den), mask, length, seed=620, check=True)
    assert np.array_equal(r.out.to_numpy(), want)
    assert not r.status_host().any() and not r.errpos_host().any() and len(r.status_host()) == 2 * length
    assert r.summaries == [_summary(pp, length, 0)] * 2 and r.summary == _summary(pp, length, 0) and r.parties is None
    for bad_num, bad_den in (([1], []), ([], [n - 1]), ([0], [n // 2])):
        nd, dd = _dev(pp, _liars(num, bad_num, 630)), _dev(pp, _liars(den, bad_den, 640))
        r = zk.d_pp(pp, nd, dd, mask, length, seed=620, check=True)
        what = (curve, l, length, bad_num, bad_den)
        assert np.array_equal(r.out.to_numpy(), want), what
        for (st, err), bad in zip(_halves(r, length), (bad_num, bad_den)):
            assert (st == (1 if bad else 0)).all() and (err == sum(1 << p for p in bad)).all(), what
        assert r.summaries == [_summary(pp, length, 1 if b else 0, b) for b in (bad_num, bad_den)], what
        # both words were repaired in place
        assert np.array_equal(nd.to_numpy().reshape(num.shape), num) and np.array_equal(dd.to_numpy().reshape(den.shape), den)


@pytest.mark.parametrize("length", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_l_plus_one_liars_in_den_fail_that_half_and_the_call_returns_what_d_pp_returns(curve, l, length):
    """a random word lands within cap of a codeword with probability about n^cap / r: every den chunk fails"""
    pp = ctx(curve, l)
    n = pp.n
    num, den = _honest(pp, length, 650 + l)
    recv = _liars(den, random.Random(l).sample(range(n), l + 1), 660)
    mask = zk.DegRedMask.sample(pp, length, 670)
    want = pp.alloc_fr(n * length)
    nu, du = _dev(pp, num), _dev(pp, recv)
    rc_want = pp.lib.zk_d_pp(pp.h, nu.ptr, du.ptr, mask.in_mask.ptr, mask.out_mask.ptr, length, 680, want.ptr, None)
    nd, dd, out = _dev(pp, num), _dev(pp, recv), pp.alloc_fr(n * length)
    st, err, summ = zk.DeviceBuffer(pp, 2 * length), zk.DeviceBuffer(pp, 8 * length), zk.DeviceBuffer(pp, 16 * (3 + n))
    rc = pp.lib.zk_d_pp_checked(pp.h, nd.ptr, dd.ptr, None, n, mask.in_mask.ptr, mask.out_mask.ptr, length, 680, out.ptr,
                                st.ptr, err.ptr, summ.ptr, None)
    assert rc == rc_want
    status = st.to_numpy(np.uint8)[:2 * length]
    assert not status[:length].any() and (status[length:] == 2).all() and not err.to_numpy(np.uint32)[:2 * length].any()
    assert [int(v) for v in summ.to_numpy(np.uint64)] == _summary(pp, length, 0) + _summary(pp, length, 2)
    # the shares went to the king as received
    assert np.array_equal(dd.to_numpy().reshape(den.shape), recv)
    if rc == 0:
        assert np.array_equal(out.to_numpy(), want.to_numpy())


def test_a_party_list_with_a_liar_equals_the_oracle_on_the_honest_shares():
    curve, l, length = "bn254", 2, 4
    pp, o = ctx(curve, l), opp(curve, l)
    n = pp.n
    numv = [v or 1 for v in rand_vec(690, length * l, o.p)]
    denv = [v or 1 for v in rand_vec(691, length * l, o.p)]
    assert all(numv) and all(denv)
    ns, ds = od.transpose(od.pack_vec(numv, o, 692)), od.transpose(od.pack_vec(denv, o, 693))
    masks = od.DegRedMask.sample(o, 1, length, 694)
    want = od.d_pp(ns, ds, masks, o, seed=695)
    dm = zk.DegRedMask(up_parties(pp, [k.in_mask for k in masks]), up_parties(pp, [k.out_mask for k in masks]))
    absent, bad = 2, 5
    S = [q for q in range(n) if q != absent]
    lie = rand_vec(696, length, o.p)
    nd = up_parties(pp, [lie if q == bad else ns[q] for q in S])
    dd = up_parties(pp, [ds[q] for q in S])
    r = zk.d_pp(pp, nd, dd, dm, length, seed=695, check=True, parties=S)
    assert down_parties(pp, r.out, n, length) == want
    (st_n, err_n), (st_d, err_d) = _halves(r, length)
    assert (st_n == 1).all() and (err_n == 1 << bad).all() and not st_d.any() and not err_d.any()
    assert r.summaries == [_summary(pp, length, 1, [bad]), _summary(pp, length, 0)] and r.parties == S
    assert down_parties(pp, nd, n - 1, length) == [ns[q] for q in S]


def test_refusals_and_the_empty_vector():
    pp = ctx("bn254", 2)
    n, l, length = pp.n, pp.l, 4
    num, den = _honest(pp, length, 700)
    nd, dd, out = _dev(pp, num), _dev(pp, den), pp.alloc_fr(n * length)
    st = zk.DeviceBuffer(pp, 2 * length)
    fn = pp.lib.zk_d_pp_checked
    assert fn(pp.h, None, None, None, n, None, None, 0, 1, None, None, None, None, None) == 0
    few = (C.c_uint32 * (2 * l))(*range(2 * l))
    assert fn(pp.h, nd.ptr, dd.ptr, few, 2 * l, None, None, length, 1, out.ptr, st.ptr, None, None, None) == 2
    bad = (C.c_uint32 * 5)(0, 1, 3, 2, 4)
    assert fn(pp.h, nd.ptr, dd.ptr, bad, 5, None, None, length, 1, out.ptr, st.ptr, None, None, None) == 4
    for args in ((None, dd.ptr, out.ptr, st.ptr), (nd.ptr, None, out.ptr, st.ptr), (nd.ptr, dd.ptr, None, st.ptr),
                 (nd.ptr, dd.ptr, out.ptr, None)):
        assert fn(pp.h, args[0], args[1], None, n, None, None, length, 1, args[2], args[3], None, None, None) == 4
    assert np.array_equal(nd.to_numpy().reshape(num.shape), num) and np.array_equal(dd.to_numpy().reshape(den.shape), den)
    # NULL errpos and summary, no masks; the context is still usable
    pp._check(fn(pp.h, nd.ptr, dd.ptr, None, n, None, None, length, 1, out.ptr, st.ptr, None, None, None))
    assert not st.to_numpy(np.uint8)[:2 * length].any()
    want = zk.d_pp(pp, nd, dd, zk.DegRedMask.zero(), length, seed=1)
    assert np.array_equal(out.to_numpy(), want.to_numpy())
