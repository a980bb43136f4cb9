"""GPU parity (through the C ABI) for zk_pss_unpack_robust_parties, the error-correcting unpack of a party list: status,
message, errpos, secrets and summary equal tests/gao_erasure_model.py exactly, on every curve and packing factor, for vectors
of 331 chunks (more than one 256-lane workgroup of stage 1, not a multiple of a wave or of the decoder's groups per wave)
that cycle through gao_erasure_model.case_list_parties, one launch per party set; plus the properties a caller relies on.
Field elements are compared as the Montgomery limbs the device holds (they are canonical): every distinct word is decoded
and encoded once."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gao_erasure_model as em
import gao_model as gm
import zksaas_amd as zk
from oracle.prng import rand_vec

from gpu_util import ctx, opp, up

CURVES = ["bn254", "bls12_381", "bls12_377"]
NCH = 331
# stage 2 runs at most 1024 workgroups of 256 / n groups (csrc/gao_impl.hpp): at l = 8 a workgroup strides from 8193 dirty
# chunks on
NCH_STRIDE = 1024 * (256 // 32) + 1
BAD_INPUT, PROTOCOL = 4, 2


def _consts(curve, l):
    o = opp(curve, l)
    return o, o.p, o.share.group_gen, o.secret.group_gen, o.curve.r_gen


@functools.lru_cache(maxsize=None)
def _model(curve, l):
    """{(k, parties): [(word, status, errpos, secrets, message)]}: the case list decoded once per (curve, l), field elements
    as limb arrays [count][nl]"""
    pp = ctx(curve, l)
    o, p, w, w2l, g = _consts(curve, l)
    by_set = {}
    for _, k, S, word in em.case_list_parties(l, p, w, 3):
        d = em.decode(word, S, k, w, p)
        sec = gm.secrets(d.message, l, g, w2l, p) if d.status != 2 else [0] * l
        by_set.setdefault((k, tuple(S)), []).append(
            (pp.fr.encode(word), d.status, d.errpos, pp.fr.encode(sec), pp.fr.encode(d.message)))
    return by_set


def _limbs(pp, buf, *shape):
    return buf.to_numpy().reshape(*shape, pp.fr.nl)


def _rows(pp, sh, nch):
    """a device vector [n][nch] -> limbs [n][nch][nl] on the host"""
    return _limbs(pp, sh, pp.n, nch)


def _subset(pp, rows, parties):
    return zk.DeviceBuffer.from_numpy(pp, rows[list(parties)])


def _check_vector(pp, cases, pick, k, S, nch):
    """one launch over the chunks cases[pick[c]]; every output against the model"""
    n, l = pp.n, pp.l
    shares = np.stack([cases[i][0] for i in pick], axis=1)                     # [|S|][nch][nl]
    r = pp.unpack_robust(zk.DeviceBuffer.from_numpy(pp, shares), nch, k, want_message=True, parties=S)
    assert r.parties == list(S)
    what = (pp.l, k, S)
    assert list(r.status_host()) == [cases[i][1] for i in pick], what
    assert list(r.errpos_host()) == [cases[i][2] for i in pick], what
    assert np.array_equal(_limbs(pp, r.secrets, nch, l), np.stack([cases[i][3] for i in pick])), what
    assert np.array_equal(_limbs(pp, r.message, k, nch), np.stack([cases[i][4] for i in pick], axis=1)), what
    want = [sum(1 for i in pick if cases[i][1] == s) for s in (0, 1, 2)]
    want += [sum((cases[i][2] >> q) & 1 for i in pick) for q in range(n)]
    assert r.summary == want, what
    assert not any(want[3 + q] for q in range(n) if q not in S)


@pytest.mark.parametrize("l", [1, 2, 4, 8])
@pytest.mark.parametrize("curve", CURVES)
def test_case_vectors_equal_the_model(curve, l):
    pp = ctx(curve, l)
    by_set = _model(curve, l)
    assert {k for k, _ in by_set} == {2 * l, 3 * l, 1, 4 * l - 1}
    assert any(len(S) < pp.n for _, S in by_set)
    for (k, S), cases in by_set.items():
        _check_vector(pp, cases, [c % len(cases) for c in range(NCH)], k, S, NCH)


def _call(pp, sh, parties, nparties, nch, k):
    """zk_pss_unpack_robust_parties with every output, the list as given (None: a NULL list)"""
    r = zk.RobustUnpack(pp, nch, k, parties)
    r.secrets, r.message = pp.alloc_fr(pp.l * nch), pp.alloc_fr(k * nch)
    r.status, r.errpos = zk.DeviceBuffer(pp, nch), zk.DeviceBuffer(pp, 4 * nch)
    r.summary_d = zk.DeviceBuffer(pp, 8 * (3 + pp.n))
    arr = None if parties is None else (C.c_uint32 * len(parties))(*parties)
    pp._check(pp.lib.zk_pss_unpack_robust_parties(pp.h, sh.ptr, arr, nparties, nch, k, r.secrets.ptr, r.message.ptr,
                                                  r.status.ptr, r.errpos.ptr, r.summary_d.ptr, None))
    return r


@pytest.mark.parametrize("l", [1, 2, 4, 8])
@pytest.mark.parametrize("curve", CURVES)
def test_all_parties_listed_equals_unpack_robust(curve, l):
    """a NULL list of n parties and the explicit full list against zk_pss_unpack_robust, output for output, on a vector
    that holds clean, corrected and failed chunks"""
    pp = ctx(curve, l)
    n = pp.n
    full = tuple(range(n))
    for k in (2 * l, 4 * l - 1):
        cases = _model(curve, l)[(k, full)]
        assert {c[1] for c in cases} == ({0, 1, 2} if k == 2 * l else {0, 2})
        sh = zk.DeviceBuffer.from_numpy(pp, np.stack([cases[c % len(cases)][0] for c in range(NCH)], axis=1))
        ref = pp.unpack_robust(sh, NCH, k, want_message=True)
        for r in (_call(pp, sh, None, n, NCH, k), _call(pp, sh, list(full), n, NCH, k),
                  pp.unpack_robust(sh, NCH, k, want_message=True, parties=full)):
            for a, b in ((r.status, ref.status), (r.errpos, ref.errpos), (r.secrets, ref.secrets), (r.message, ref.message),
                         (r.summary_d, ref.summary_d)):
                assert np.array_equal(a.to_numpy(np.uint8), b.to_numpy(np.uint8)), (curve, l, k)


@pytest.mark.parametrize("l", [1, 2, 4, 8])
@pytest.mark.parametrize("curve", CURVES)
def test_clean_shares_with_absent_parties(curve, l):
    """every single party absent, and l parties absent: the packed secrets, and zk_pss_unpack2's with the same list wherever
    unpack2 takes it (it needs more than 4l - 2 parties, pss.rs:183-186)"""
    pp = ctx(curve, l)
    n, p = pp.n, opp(curve, l).p
    sec = up(pp, rand_vec(140 + l, NCH * l, p))
    rows = _rows(pp, pp.pack(sec, NCH, seed=19), NCH)
    want = _limbs(pp, sec, NCH, l)
    rnd = random.Random(l)
    lists = [[q for q in range(n) if q != e] for e in range(n)]
    lists += [sorted(rnd.sample(range(n), n - l)) for _ in range(3)] + [list(range(l, n)), list(range(n - l))]
    for S in lists:
        buf = _subset(pp, rows, S)
        r = pp.unpack_robust(buf, NCH, parties=S)
        assert np.array_equal(_limbs(pp, r.secrets, NCH, l), want), (curve, l, S)
        assert not r.status_host().any() and not r.errpos_host().any()
        assert r.summary == [NCH, 0, 0] + [0] * n
        if len(S) > 4 * l - 2:
            assert np.array_equal(_limbs(pp, pp.unpack2(buf, NCH, S), NCH, l), want), (curve, l, S)
    # squared shares have degree <= 4l - 2, dimension 4l - 1: the largest list that dimension allows is all n parties
    sq = [[int(v) * int(v) % p for v in pp.fr.decode(row)] for row in rows]
    buf = pp.upload_fr([v for row in sq for v in row])
    r2 = pp.unpack_robust(buf, NCH, 4 * l - 1, parties=list(range(n)))
    assert np.array_equal(r2.secrets.to_numpy(), pp.unpack2(buf, NCH).to_numpy())
    assert pp.download_fr(r2.secrets) == [v * v % p for v in pp.download_fr(sec)]
    assert not r2.status_host().any()
    with pytest.raises(zk.ZkError) as e:
        pp.unpack_robust(_subset(pp, rows, range(1, n)), NCH, 4 * l - 1, parties=list(range(1, n)))
    assert e.value.code == PROTOCOL


def _raw(rng, count):          # any limbs below 2^252 are a field element in Montgomery form
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


@pytest.mark.parametrize("l", [2, 4, 8])
def test_a_liar_beside_an_absent_party_is_named_by_id(l):
    pp = ctx("bn254", l)
    n = pp.n
    rng = np.random.default_rng(l)
    sec = zk.DeviceBuffer.from_numpy(pp, _raw(rng, NCH * l))
    rows = _rows(pp, pp.pack(sec, NCH, seed=20), NCH)
    want = _limbs(pp, sec, NCH, l)
    for absent, liar in ((0, 1), (n // 2, n - 1), (n - 1, 0), (3, 2)):
        cur = rows.copy()
        cur[liar] = _raw(rng, NCH)
        S = [q for q in range(n) if q != absent]
        r = pp.unpack_robust(_subset(pp, cur, S), NCH, parties=S)
        assert set(r.status_host()) == {1} and set(r.errpos_host()) == {1 << liar}, (l, absent, liar)
        tally = [0, NCH, 0] + [0] * n
        tally[3 + liar] = NCH
        assert r.summary == tally
        assert np.array_equal(_limbs(pp, r.secrets, NCH, l), want)
        # the liar listed absent (with the dropout, and alone): clean everywhere
        for S2 in ([q for q in S if q != liar], [q for q in range(n) if q != liar]):
            r = pp.unpack_robust(_subset(pp, cur, S2), NCH, parties=S2)
            assert not r.status_host().any() and not r.errpos_host().any(), (l, absent, liar)
            assert r.summary == [NCH, 0, 0] + [0] * n
            assert np.array_equal(_limbs(pp, r.secrets, NCH, l), want)


@pytest.mark.parametrize("l", [1, 2, 4, 8])
def test_cap_plus_one_liars_never_pass_as_clean(l):
    pp = ctx("bls12_377", l)
    o, p, w, w2l, g = _consts("bls12_377", l)
    n, k = pp.n, 2 * l
    rows = _rows(pp, pp.pack(up(pp, rand_vec(170 + l, NCH * l, p)), NCH, seed=21), NCH)
    S = [q for q in range(n) if q != n // 2]
    cap = (len(S) - k) // 2
    cur = [pp.fr.decode(rows[q]) for q in S]
    for i in random.Random(l).sample(range(len(S)), cap + 1):
        cur[i] = rand_vec(180 + i, NCH, p)
    r = pp.unpack_robust(pp.upload_fr([v for row in cur for v in row]), NCH, k, want_message=True, parties=S)
    status, errpos = list(r.status_host()), list(r.errpos_host())
    sec, msg = pp.download_fr(r.secrets), pp.download_fr(r.message)
    assert 0 not in status
    xs = [pow(w, q, p) for q in S]
    for c in range(NCH):
        h = [msg[j * NCH + c] for j in range(k)]
        if status[c] == 2:
            assert sec[c * l:(c + 1) * l] == [0] * l and errpos[c] == 0 and h == [0] * k
        else:
            # the self-check: the message differs from the listed shares exactly at errpos
            assert errpos[c] == sum(1 << q for q, x, row in zip(S, xs, cur) if gm.poly_eval(h, x, p) != row[c])
            assert 1 <= bin(errpos[c]).count("1") <= cap
            assert sec[c * l:(c + 1) * l] == gm.secrets(h, l, g, w2l, p)
    assert r.summary[:3] == [0, status.count(1), status.count(2)]


def test_dirty_list_longer_than_one_sweep_of_stage_2_with_an_absent_party():
    """8193 dirty chunks at l = 8: the decoder's workgroups walk the list with their grid stride; a handful of words the
    model decoded, repeated"""
    l, k = 8, 16
    pp = ctx("bn254", l)
    S = tuple(q for q in range(pp.n) if q != pp.n // 2)
    dirty = _model("bn254", l)[(k, S)]
    cases = [c for c in dirty if c[1] == 1][:4] + [c for c in dirty if c[1] == 2][:3]
    assert [c[1] for c in cases] == [1] * 4 + [2] * 3
    _check_vector(pp, cases, [c % len(cases) for c in range(NCH_STRIDE)], k, S, NCH_STRIDE)


def test_empty_vector_null_outputs_and_refusals():
    pp = ctx("bn254", 2)
    n, p = pp.n, opp("bn254", 2).p
    fn = pp.lib.zk_pss_unpack_robust_parties
    S = [0, 1, 2, 4, 5, 6, 7]
    ids = (C.c_uint32 * len(S))(*S)
    r = pp.unpack_robust(pp.alloc_fr(0), 0, parties=S)
    assert r.summary == [0] * (3 + n) and len(r.status_host()) == 0
    assert fn(pp.h, None, ids, len(S), 0, 4, None, None, None, None, None, None) == 0
    secrets = rand_vec(195, 7 * 2, p)
    rows = _rows(pp, pp.pack(up(pp, secrets), 7, seed=22), 7)
    sh = _subset(pp, rows, S)
    # only the status is mandatory; each optional output alone
    st = zk.DeviceBuffer(pp, 7)
    pp._check(fn(pp.h, sh.ptr, ids, len(S), 7, 4, None, None, st.ptr, None, None, None))
    assert not st.to_numpy(np.uint8).any()
    sec, msg, err, summ = pp.alloc_fr(14), pp.alloc_fr(28), zk.DeviceBuffer(pp, 28), zk.DeviceBuffer(pp, 8 * (3 + n))
    pp._check(fn(pp.h, sh.ptr, ids, len(S), 7, 4, sec.ptr, None, st.ptr, None, None, None))
    assert pp.download_fr(sec) == secrets
    pp._check(fn(pp.h, sh.ptr, ids, len(S), 7, 4, None, msg.ptr, st.ptr, err.ptr, summ.ptr, None))
    full = pp.unpack_robust(sh, 7, want_message=True, parties=S)
    assert np.array_equal(msg.to_numpy(), full.message.to_numpy()) and not err.to_numpy(np.uint32).any()
    assert [int(v) for v in summ.to_numpy(np.uint64)] == [7, 0, 0] + [0] * n
    # refusals: the list, the dimension, the pointers -> BAD_INPUT; too few shares -> PROTOCOL
    for bad in ([0, 1, 2, 2, 4, 5, 6], [0, 1, 2, 4, 3, 5, 6], [0, 1, 2, 4, 5, 6, 8], [1, 0, 2, 3, 4, 5, 6]):
        with pytest.raises(zk.ZkError) as e:
            pp.unpack_robust(sh, 7, parties=bad)
        assert e.value.code == BAD_INPUT, bad
    for bad_k in (0, -1, n, n + 5):
        with pytest.raises(zk.ZkError) as e:
            pp.unpack_robust(sh, 7, bad_k, parties=S)
        assert e.value.code == BAD_INPUT
    for count in (0, -1, n + 1):
        assert fn(pp.h, sh.ptr, None, count, 7, 4, None, None, st.ptr, None, None, None) == BAD_INPUT
    for args in ((None, st.ptr), (sh.ptr, None)):
        assert fn(pp.h, args[0], ids, len(S), 7, 4, None, None, args[1], None, None, None) == BAD_INPUT
    for few, k in (([0, 1, 2, 4], 4), ([0, 1, 2], 4), (S, 7), ([3], 1)):
        with pytest.raises(zk.ZkError) as e:
            pp.unpack_robust(sh, 7, k, parties=few)
        assert e.value.code == PROTOCOL, (few, k)
    assert fn(pp.h, None, ids, 4, 0, 4, None, None, None, None, None, None) == PROTOCOL
    # a NULL list of fewer than n parties stands for 0 .. nparties - 1
    head = list(range(6))
    r = _call(pp, _subset(pp, rows, head), None, 6, 7, 4)
    assert pp.download_fr(r.secrets) == secrets and not r.status_host().any()
    # the context is still usable
    assert pp.download_fr(pp.unpack_robust(sh, 7, parties=S).secrets) == secrets
