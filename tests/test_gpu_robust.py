"""GPU parity (through the C ABI) for zk_pss_unpack_robust, the error-correcting unpack: status, message, errpos, secrets and
summary equal tests/gao_model.py exactly, on every curve and packing factor, for vectors of 331 chunks (more than one
256-lane workgroup of stage 1, not a multiple of a wave or of the decoder's groups per wave) that cycle through
gao_model.case_list; plus the properties a caller relies on."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gao_model as gm
import zksaas_amd as zk
from oracle.prng import rand_vec

from gpu_util import ctx, opp, up, up_parties

CURVES = ["bn254", "bls12_381", "bls12_377"]
NCH = 331
# stage 2 runs at most GAO_STAGE2_GRID = 1024 workgroups of 256 / n groups (csrc/gao_impl.hpp); at l = 8 (n = 32) that is
# 8192 dirty chunks per sweep, so 8193 dirty chunks is the smallest count at which a workgroup strides to a second chunk
STAGE2_GRID = 1024
NCH_STRIDE = STAGE2_GRID * (256 // 32) + 1


def _consts(curve, l):
    o = opp(curve, l)
    return o, o.p, o.share.group_gen, o.secret.group_gen, o.curve.r_gen


@functools.lru_cache(maxsize=None)
def _model(curve, l):
    """{k: [(word, Decoded, secrets)]} over the case list, decoded once per (curve, l)"""
    o, p, w, w2l, g = _consts(curve, l)
    by_k = {}
    for _, k, y in gm.case_list(l, p, w, 3):
        d = gm.decode(y, k, w, p)
        sec = gm.secrets(d.message, l, g, w2l, p) if d.status != 2 else [0] * l
        by_k.setdefault(k, []).append((y, d, sec))
    return by_k


def _columns(words, n):
    """chunk-major words -> party-major rows [n][len(words)]"""
    return [[y[p] for y in words] for p in range(n)]


def _fields(pp, r, k):
    nch = r.nchunks
    sec = pp.download_fr(r.secrets, nch * pp.l)
    msg = pp.download_fr(r.message, k * nch) if r.message is not None else None
    return list(r.status_host()), list(r.errpos_host()), sec, msg


@pytest.mark.parametrize("l", [1, 2, 4, 8])
@pytest.mark.parametrize("curve", CURVES)
def test_case_vectors_equal_the_model(curve, l):
    pp = ctx(curve, l)
    n = pp.n
    by_k = _model(curve, l)
    assert sorted(by_k) == sorted({2 * l, 3 * l, 4 * l - 1, 1, n - 1})
    for k, cases in by_k.items():
        pick = [cases[c % len(cases)] for c in range(NCH)]
        r = pp.unpack_robust(up_parties(pp, _columns([c[0] for c in pick], n)), NCH, k, want_message=True)
        status, errpos, sec, msg = _fields(pp, r, k)
        assert status == [c[1].status for c in pick], (curve, l, k)
        assert errpos == [c[1].errpos for c in pick], (curve, l, k)
        assert sec == [v for c in pick for v in c[2]], (curve, l, k)
        assert msg == [c[1].message[j] for j in range(k) for c in pick], (curve, l, k)
        want_sum = [sum(1 for c in pick if c[1].status == s) for s in (0, 1, 2)]
        want_sum += [sum((c[1].errpos >> q) & 1 for c in pick) for q in range(n)]
        assert r.summary == want_sum, (curve, l, k)


@pytest.mark.parametrize("l", [1, 2, 4, 8])
@pytest.mark.parametrize("curve", CURVES)
def test_clean_shares_equal_unpack_and_unpack2(curve, l):
    pp = ctx(curve, l)
    o, p = opp(curve, l), opp(curve, l).p
    secrets = rand_vec(40 + l, NCH * l, p)
    sh = pp.pack(up(pp, secrets), NCH, seed=9)
    r = pp.unpack_robust(sh, NCH)
    assert pp.download_fr(r.secrets) == pp.download_fr(pp.unpack(sh, NCH)) == secrets
    assert not r.status_host().any() and not r.errpos_host().any()
    assert r.summary == [NCH, 0, 0] + [0] * pp.n
    # squared shares: degree <= 4l - 2, dimension 4l - 1
    rows = np.asarray(pp.download_fr(sh), dtype=object).reshape(pp.n, NCH)
    sq = [[int(v) * int(v) % p for v in row] for row in rows]
    buf = up_parties(pp, sq)
    r2 = pp.unpack_robust(buf, NCH, 4 * l - 1)
    assert pp.download_fr(r2.secrets) == pp.download_fr(pp.unpack2(buf, NCH)) == [v * v % p for v in secrets]
    assert not r2.status_host().any()


@pytest.mark.parametrize("l", [1, 2, 4, 8])
def test_one_bad_party_is_named_and_corrected(l):
    pp = ctx("bn254", l)
    p = opp("bn254", l).p
    secrets = rand_vec(50 + l, NCH * l, p)
    rows = np.asarray(pp.download_fr(pp.pack(up(pp, secrets), NCH, seed=10)), dtype=object).reshape(pp.n, NCH)
    for bad in sorted({0, pp.n // 2 + 1, pp.n - 1}):
        cur = [list(map(int, row)) for row in rows]
        cur[bad] = rand_vec(60 + bad, NCH, p)
        r = pp.unpack_robust(up_parties(pp, cur), NCH)
        assert set(r.status_host()) == {1}
        assert set(r.errpos_host()) == {1 << bad}
        want = [0, NCH, 0] + [0] * pp.n
        want[3 + bad] = NCH
        assert r.summary == want
        assert pp.download_fr(r.secrets) == secrets


@pytest.mark.parametrize("l", [1, 2, 4, 8])
def test_too_many_bad_parties_never_pass_as_clean(l):
    pp = ctx("bls12_377", l)
    o, p, w, w2l, g = _consts("bls12_377", l)
    n, k = pp.n, 2 * l
    secrets = rand_vec(70 + l, NCH * l, p)
    rows = np.asarray(pp.download_fr(pp.pack(up(pp, secrets), NCH, seed=11)), dtype=object).reshape(n, NCH)
    cur = [list(map(int, row)) for row in rows]
    for bad in random.Random(l).sample(range(n), l + 1):
        cur[bad] = rand_vec(80 + bad, NCH, p)
    r = pp.unpack_robust(up_parties(pp, cur), NCH, want_message=True)
    status, errpos, sec, msg = _fields(pp, r, k)
    assert 0 not in status
    for c in range(NCH):
        if status[c] == 2:
            assert sec[c * l:(c + 1) * l] == [0] * l and errpos[c] == 0
            assert [msg[j * NCH + c] for j in range(k)] == [0] * k
        else:
            # the self-check: re-encoding the message differs from the received word exactly at errpos
            h = [msg[j * NCH + c] for j in range(k)]
            code = gm.encode(h, n, w, p)
            assert errpos[c] == sum(1 << q for q in range(n) if code[q] != cur[q][c])
            assert 1 <= bin(errpos[c]).count("1") <= (n - k) // 2
            assert sec[c * l:(c + 1) * l] == gm.secrets(h, l, g, w2l, p)
    assert r.summary[:3] == [0, status.count(1), status.count(2)]


def test_dirty_list_longer_than_one_sweep_of_stage_2():
    """every chunk dirty, NCH_STRIDE of them at l = 8: the decoder's workgroups walk the list with their grid stride"""
    l = 8
    pp = ctx("bn254", l)
    nch, bad = NCH_STRIDE, 5
    rng = np.random.default_rng(90)

    def raw(count):          # any limbs below the modulus are a field element in Montgomery form: 2^252 < r
        a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 60) - 1)
        return a

    sec = zk.DeviceBuffer.from_numpy(pp, raw(nch * l))
    rows = pp.pack(sec, nch, seed=12).to_numpy().reshape(pp.n, nch, 4)
    rows[bad] = raw(nch)
    sh = zk.DeviceBuffer.from_numpy(pp, rows)
    r = pp.unpack_robust(sh, nch)
    assert (r.status_host() == 1).all() and (r.errpos_host() == 1 << bad).all()
    want = [0, nch, 0] + [0] * pp.n
    want[3 + bad] = nch
    assert r.summary == want
    assert np.array_equal(r.secrets.to_numpy(), sec.to_numpy())


def test_empty_vector_null_outputs_and_bad_dimension():
    pp = ctx("bn254", 2)
    p = opp("bn254", 2).p
    r = pp.unpack_robust(pp.alloc_fr(0), 0)
    assert r.summary == [0] * (3 + pp.n) and len(r.status_host()) == 0
    assert pp.lib.zk_pss_unpack_robust(pp.h, None, 0, 4, None, None, None, None, None, None) == 0
    # only the status is mandatory
    secrets = rand_vec(95, 7 * 2, p)
    sh = pp.pack(up(pp, secrets), 7, seed=13)
    st = zk.DeviceBuffer(pp, 7)
    pp._check(pp.lib.zk_pss_unpack_robust(pp.h, sh.ptr, 7, 4, None, None, st.ptr, None, None, None))
    assert not st.to_numpy(np.uint8).any()
    for bad_k in (0, -1, pp.n, pp.n + 5):
        with pytest.raises(zk.ZkError) as e:
            pp.unpack_robust(sh, 7, bad_k)
        assert e.value.code == 4
    for args in ((None, st.ptr), (sh.ptr, None)):
        assert pp.lib.zk_pss_unpack_robust(pp.h, args[0], 7, 4, None, None, args[1], None, None, None) == 4
    # the context is still usable
    assert pp.download_fr(pp.unpack_robust(sh, 7).secrets) == secrets
