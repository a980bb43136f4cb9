"""GPU parity (through the C ABI) for zk_pss_repair_parties, the repair of the shares of a party list: status, errpos and
summary equal zk_pss_unpack_robust_parties' on a copy of the input and tests/gao_erasure_model.py; the share matrix after the
call equals the model's repaired matrix element for element (so what must stay untouched is untouched), for vectors of 331
chunks (more than one 256-lane workgroup of the scan, not a multiple of a wave or of the decoder's groups per wave: the last
wave is partly live) that cycle through gao_erasure_model.case_list_parties, one launch per party set; plus the properties a
caller relies on.  Field elements are compared as the Montgomery limbs the device holds (they are canonical)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gao_erasure_model as em
import gao_model as gm
import zksaas_amd as zk

from gpu_util import ctx, opp

CONFIGS = [("bn254", 1), ("bn254", 2), ("bn254", 4), ("bn254", 8), ("bls12_381", 2), ("bls12_377", 2)]
IDS = ["%s_l%d" % c for c in CONFIGS]
NCH = 331
# stage 2 runs at most 1024 workgroups of 256 / n groups (csrc/gao_impl.hpp): a workgroup strides to a second chunk from
# 1024 * (256 // n) + 1 dirty chunks on, which is smallest at l = 8 (n = 32)
NCH_STRIDE = 1024 * (256 // 32) + 1
BAD_INPUT, PROTOCOL = 4, 2


@functools.lru_cache(maxsize=None)
def _model(curve, l):
    """{(k, parties): [(word, status, errpos, repaired word)]}: the case list decoded once per (curve, l), words as limb
    arrays [|S|][nl]"""
    pp, o = ctx(curve, l), opp(curve, l)
    p, w = o.p, o.share.group_gen
    by_set = {}
    for _, k, S, word in em.case_list_parties(l, p, w, 7):
        d = em.decode(word, S, k, w, p)
        fixed = list(word)
        if d.status == 1:
            for i, q in enumerate(S):
                if (d.errpos >> q) & 1:
                    fixed[i] = gm.poly_eval(d.message, pow(w, q, p), p)
        by_set.setdefault((k, tuple(S)), []).append((pp.fr.encode(word), d.status, d.errpos, pp.fr.encode(fixed)))
    return by_set


def _dev(pp, arr):
    return zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(arr))


def _verdicts(r):
    return list(r.status_host()), list(r.errpos_host()), r.summary


def _check_vector(pp, cases, pick, k, S, nch, twice=True):
    """one repair over the chunks cases[pick[c]]; every output against the model and against unpack_robust with the list"""
    n = pp.n
    shares = np.stack([cases[i][0] for i in pick], axis=1)                     # [|S|][nch][nl]
    what = (pp.l, k, S)
    robust = pp.unpack_robust(_dev(pp, shares), nch, k, parties=S)
    sh = _dev(pp, shares)
    r = pp.repair(sh, nch, k, parties=S)
    assert r.parties == list(S) and r.out is sh
    status, errpos, summary = _verdicts(r)
    assert (status, errpos, summary) == _verdicts(robust), what
    assert status == [cases[i][1] for i in pick], what
    assert errpos == [cases[i][2] for i in pick], what
    want = [sum(1 for i in pick if cases[i][1] == s) for s in (0, 1, 2)]
    want += [sum((cases[i][2] >> q) & 1 for i in pick) for q in range(n)]
    assert summary == want, what
    assert not any(want[3 + q] for q in range(n) if q not in S)
    fixed = np.stack([cases[i][3] for i in pick], axis=1)
    got = sh.to_numpy().reshape(fixed.shape)
    assert np.array_equal(got, fixed), what
    if not twice:
        return
    # a second repair: the corrected chunks are clean now, the failed ones fail as before, no byte changes
    r2 = pp.repair(sh, nch, k, parties=S)
    status2, errpos2, summary2 = _verdicts(r2)
    assert status2 == [0 if s == 1 else s for s in status] and not any(errpos2), what
    assert summary2 == [want[0] + want[1], 0, want[2]] + [0] * n, what
    assert np.array_equal(sh.to_numpy().reshape(fixed.shape), fixed), what


@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_case_vectors_equal_the_model_and_a_second_repair_finds_them_clean(curve, l):
    pp = ctx(curve, l)
    by_set = _model(curve, l)
    assert {k for k, _ in by_set} == {2 * l, 3 * l, 1, 4 * l - 1}
    assert any(len(S) < pp.n for _, S in by_set)
    seen = set()
    for (k, S), cases in by_set.items():
        _check_vector(pp, cases, [c % len(cases) for c in range(NCH)], k, S, NCH)
        if len(S) < pp.n:
            seen |= {c[1] for c in cases}
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_all_parties_listed_equals_repair_byte_for_byte(curve, l):
    """a NULL list of n parties and the explicit full list against zk_pss_repair: the verdicts and the matrix"""
    pp = ctx(curve, l)
    n = pp.n
    full = tuple(range(n))
    fn = pp.lib.zk_pss_repair_parties
    for k in (2 * l, 4 * l - 1):
        cases = _model(curve, l)[(k, full)]
        assert {c[1] for c in cases} == ({0, 1, 2} if k == 2 * l else {0, 2})
        shares = np.stack([cases[c % len(cases)][0] for c in range(NCH)], axis=1)
        ref_sh = _dev(pp, shares)
        ref = pp.repair(ref_sh, NCH, k)
        for ids in (None, (C.c_uint32 * n)(*full)):
            sh = _dev(pp, shares)
            st, err, summ = zk.DeviceBuffer(pp, NCH), zk.DeviceBuffer(pp, 4 * NCH), zk.DeviceBuffer(pp, 8 * (3 + n))
            pp._check(fn(pp.h, sh.ptr, ids, n, NCH, k, st.ptr, err.ptr, summ.ptr, None))
            for a, b in ((st, ref.status), (err, ref.errpos), (summ, ref.summary_d), (sh, ref_sh)):
                assert np.array_equal(a.to_numpy(np.uint8), b.to_numpy(np.uint8)), (curve, l, k)


def _raw(rng, count):          # any limbs below 2^252 are a field element in Montgomery form
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def _honest(pp, nch, seed):
    sec = zk.DeviceBuffer.from_numpy(pp, _raw(np.random.default_rng(seed), nch * pp.l))
    return pp.pack(sec, nch, seed=seed).to_numpy().reshape(pp.n, nch, 4).copy()


@pytest.mark.parametrize("l", [2, 4, 8])
def test_a_liar_beside_an_absent_party_is_named_by_id_and_written_at_its_row(l):
    pp = ctx("bn254", l)
    n = pp.n
    rng = np.random.default_rng(l)
    rows = _honest(pp, NCH, 30 + l)
    for absent, liar in ((0, 1), (n // 2, n - 1), (n - 1, 0), (3, 2)):
        cur = rows.copy()
        cur[liar] = _raw(rng, NCH)
        S = [q for q in range(n) if q != absent]
        sh = _dev(pp, cur[S])
        r = pp.repair(sh, NCH, parties=S)
        assert set(r.status_host()) == {1} and set(r.errpos_host()) == {1 << liar}, (l, absent, liar)
        tally = [0, NCH, 0] + [0] * n
        tally[3 + liar] = NCH
        assert r.summary == tally
        # row S.index(liar) holds the honest share again -- with absent < liar that is not row `liar`; no other row changed
        assert np.array_equal(sh.to_numpy().reshape(n - 1, NCH, 4), rows[S]), (l, absent, liar)
        # the liar listed absent (with the dropout, and alone): clean everywhere, nothing written
        for S2 in ([q for q in S if q != liar], [q for q in range(n) if q != liar]):
            sh = _dev(pp, cur[S2])
            r = pp.repair(sh, NCH, parties=S2)
            assert not r.status_host().any() and not r.errpos_host().any(), (l, absent, liar)
            assert r.summary == [NCH, 0, 0] + [0] * n
            assert np.array_equal(sh.to_numpy().reshape(len(S2), NCH, 4), cur[S2])


@pytest.mark.parametrize("l", [1, 2, 4, 8])
def test_cap_plus_one_liars_never_pass_as_clean_and_write_nothing(l):
    """a random word lands within cap of a codeword with probability about n^cap / r: every chunk fails"""
    pp = ctx("bls12_377", l)
    n, k = pp.n, 2 * l
    rows = _honest(pp, NCH, 40 + l)
    S = [q for q in range(n) if q != n // 2]
    cap = (len(S) - k) // 2
    cur = rows[S].copy()
    rng = np.random.default_rng(50 + l)
    for i in random.Random(l).sample(range(len(S)), cap + 1):
        cur[i] = _raw(rng, NCH)
    sh = _dev(pp, cur)
    r = pp.repair(sh, NCH, k, parties=S)
    assert (r.status_host() == 2).all() and not r.errpos_host().any()
    assert r.summary == [0, 0, NCH] + [0] * n
    assert np.array_equal(sh.to_numpy().reshape(cur.shape), cur)


def test_dirty_list_longer_than_one_sweep_of_stage_2_with_an_absent_party():
    """8193 dirty chunks at l = 8: the decoder's workgroups walk the list with their grid stride, the store sits in that
    loop; a handful of words the model decoded, repeated"""
    l, k = 8, 16
    pp = ctx("bn254", l)
    S = tuple(q for q in range(pp.n) if q != pp.n // 2)
    dirty = _model("bn254", l)[(k, S)]
    cases = [c for c in dirty if c[1] == 1][:4] + [c for c in dirty if c[1] == 2][:3]
    assert [c[1] for c in cases] == [1] * 4 + [2] * 3
    _check_vector(pp, cases, [c % len(cases) for c in range(NCH_STRIDE)], k, S, NCH_STRIDE, twice=False)


def test_empty_vector_null_outputs_and_refusals():
    pp = ctx("bn254", 2)
    n = pp.n
    fn = pp.lib.zk_pss_repair_parties
    S = [0, 1, 2, 4, 5, 6, 7]
    ids = (C.c_uint32 * len(S))(*S)
    r = pp.repair(pp.alloc_fr(0), 0, parties=S)
    assert r.summary == [0] * (3 + n) and len(r.status_host()) == 0
    assert fn(pp.h, None, ids, len(S), 0, 4, None, None, None, None) == 0
    rows = _honest(pp, 7, 60)
    recv = rows[S].copy()
    recv[3, 5] = rows[2, 1]                 # row 3 is party 4
    sh = _dev(pp, recv)
    # only the status is mandatory: errpos and summary NULL, on a vector with one wrong share
    st = zk.DeviceBuffer(pp, 7)
    pp._check(fn(pp.h, sh.ptr, ids, len(S), 7, 4, st.ptr, None, None, None))
    assert list(st.to_numpy(np.uint8)[:7]) == [0, 0, 0, 0, 0, 1, 0]
    assert np.array_equal(sh.to_numpy().reshape(recv.shape), rows[S])
    # refusals: the list, the dimension, the pointers -> BAD_INPUT; too few shares -> PROTOCOL; the shares stay as they were
    sh = _dev(pp, recv)
    for bad in ([0, 1, 2, 2, 4, 5, 6], [0, 1, 2, 4, 3, 5, 6], [0, 1, 2, 4, 5, 6, 8], [1, 0, 2, 3, 4, 5, 6]):
        with pytest.raises(zk.ZkError) as e:
            pp.repair(sh, 7, parties=bad)
        assert e.value.code == BAD_INPUT, bad
    for bad_k in (0, -1, n, n + 5):
        with pytest.raises(zk.ZkError) as e:
            pp.repair(sh, 7, bad_k, parties=S)
        assert e.value.code == BAD_INPUT
    for count in (0, -1, n + 1):
        assert fn(pp.h, sh.ptr, None, count, 7, 4, st.ptr, None, None, None) == BAD_INPUT
    for args in ((None, st.ptr), (sh.ptr, None)):
        assert fn(pp.h, args[0], ids, len(S), 7, 4, args[1], None, None, None) == BAD_INPUT
    for few, k in (([0, 1, 2, 4], 4), ([0, 1, 2], 4), (S, 7), ([3], 1)):
        with pytest.raises(zk.ZkError) as e:
            pp.repair(sh, 7, k, parties=few)
        assert e.value.code == PROTOCOL, (few, k)
    assert fn(pp.h, None, ids, 4, 0, 4, None, None, None, None) == PROTOCOL
    assert np.array_equal(sh.to_numpy().reshape(recv.shape), recv)
    # a NULL list of fewer than n parties stands for 0 .. nparties - 1
    head = rows[:6].copy()
    head[5, 0] = rows[0, 0]
    hd = _dev(pp, head)
    pp._check(fn(pp.h, hd.ptr, None, 6, 7, 4, st.ptr, None, None, None))
    assert list(st.to_numpy(np.uint8)[:7]) == [1, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(hd.to_numpy().reshape(head.shape), rows[:6])
    # the context is still usable
    r = pp.repair(sh, 7, parties=S)
    assert r.summary == [6, 1, 0] + [0, 0, 0, 0, 1, 0, 0, 0]
    assert np.array_equal(sh.to_numpy().reshape(recv.shape), rows[S])
