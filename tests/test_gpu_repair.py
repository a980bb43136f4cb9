"""GPU parity (through the C ABI) for zk_pss_repair: status, errpos and summary equal zk_pss_unpack_robust's on a copy of the
input and tests/gao_model.py; the share matrix after the call equals the model's repaired matrix element for element (so
what must stay untouched is untouched), on every curve and packing factor, for vectors of 331 chunks (more than one
workgroup of the scan, not a multiple of a wave or of the decoder's groups per wave) that cycle through
gao_model.case_list; plus the properties a caller relies on."""
import functools

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
NCH_STRIDE = 1024 * (256 // 32) + 1


@functools.lru_cache(maxsize=None)
def _model(curve, l):
    """{k: [(word, Decoded, secrets, repaired word)]} over the case list, decoded once per (curve, l)"""
    o = opp(curve, l)
    p, w, w2l, g, n = o.p, o.share.group_gen, o.secret.group_gen, o.curve.r_gen, 4 * l
    by_k = {}
    for _, k, y in gm.case_list(l, p, w, 5):
        d = gm.decode(y, k, w, p)
        sec = gm.secrets(d.message, l, g, w2l, p) if d.status != 2 else None
        fixed = list(y)
        if d.status == 1:
            code = gm.encode(gm.trim(d.message), n, w, p)
            for q in range(n):
                if (d.errpos >> q) & 1:
                    fixed[q] = code[q]
        by_k.setdefault(k, []).append((y, d, sec, fixed))
    return by_k


def _columns(words, n):
    """chunk-major words -> party-major rows [n][len(words)]"""
    return [[y[p] for y in words] for p in range(n)]


def _verdicts(r):
    return list(r.status_host()), list(r.errpos_host()), r.summary


@pytest.mark.parametrize("l", [1, 2, 4, 8])
@pytest.mark.parametrize("curve", CURVES)
def test_case_vectors_equal_the_model_and_a_second_repair_finds_them_clean(curve, l):
    pp = ctx(curve, l)
    n = pp.n
    by_k = _model(curve, l)
    assert sorted(by_k) == sorted({2 * l, 3 * l, 4 * l - 1, 1, n - 1})
    for k, cases in by_k.items():
        pick = [cases[c % len(cases)] for c in range(NCH)]
        rows = _columns([c[0] for c in pick], n)
        sh = up_parties(pp, rows)
        robust = pp.unpack_robust(up_parties(pp, rows), NCH, k)
        r = pp.repair(sh, NCH, k)
        status, errpos, summary = _verdicts(r)
        assert (status, errpos, summary) == _verdicts(robust), (curve, l, k)
        assert status == [c[1].status for c in pick], (curve, l, k)
        assert errpos == [c[1].errpos for c in pick], (curve, l, k)
        want_sum = [sum(1 for c in pick if c[1].status == s) for s in (0, 1, 2)]
        want_sum += [sum((c[1].errpos >> q) & 1 for c in pick) for q in range(n)]
        assert summary == want_sum, (curve, l, k)
        fixed = pp.download_fr(sh, n * NCH)
        assert fixed == [v for row in _columns([c[3] for c in pick], n) for v in row], (curve, l, k)
        # a second repair: the corrected chunks are clean now, the failed ones fail as before, nothing is written
        r2 = pp.repair(sh, NCH, k)
        status2, errpos2, summary2 = _verdicts(r2)
        assert status2 == [0 if s == 1 else s for s in status] and not any(errpos2), (curve, l, k)
        assert summary2 == [want_sum[0] + want_sum[1], 0, want_sum[2]] + [0] * n, (curve, l, k)
        assert pp.download_fr(sh, n * NCH) == fixed, (curve, l, k)
        # the plain unpacks on the repaired matrix: zk_pss_unpack reads words of degree < 2l, zk_pss_unpack2 any degree < n
        sec = pp.download_fr(pp.unpack(sh, NCH) if k <= 2 * l else pp.unpack2(sh, NCH), NCH * l)
        for c, case in enumerate(pick):
            if case[1].status != 2:
                assert sec[c * l:(c + 1) * l] == case[2], (curve, l, k, c)


def test_dirty_list_longer_than_one_sweep_of_stage_2():
    """every chunk dirty, NCH_STRIDE of them at l = 8: the repair store sits in the decoder's grid-stride loop"""
    l = 8
    pp = ctx("bn254", l)
    nch, bad = NCH_STRIDE, 5
    rng = np.random.default_rng(91)

    def raw(count):          # any limbs below the modulus are a field element in Montgomery form: 2^252 < r
        a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 60) - 1)
        return a

    honest = pp.pack(zk.DeviceBuffer.from_numpy(pp, raw(nch * l)), nch, seed=14).to_numpy().reshape(pp.n, nch, 4)
    rows = honest.copy()
    rows[bad] = raw(nch)
    sh = zk.DeviceBuffer.from_numpy(pp, rows)
    r = pp.repair(sh, nch)
    assert (r.status_host() == 1).all() and (r.errpos_host() == 1 << bad).all()
    want = [0, nch, 0] + [0] * pp.n
    want[3 + bad] = nch
    assert r.summary == want
    assert np.array_equal(sh.to_numpy().reshape(pp.n, nch, 4), honest)


def test_empty_vector_null_outputs_and_bad_dimension():
    pp = ctx("bn254", 2)
    p = opp("bn254", 2).p
    r = pp.repair(pp.alloc_fr(0), 0)
    assert r.summary == [0] * (3 + pp.n) and len(r.status_host()) == 0
    assert pp.lib.zk_pss_repair(pp.h, None, 0, 4, None, None, None, None) == 0
    # only the status is mandatory: errpos and summary NULL, on a vector with one wrong share
    secrets = rand_vec(96, 7 * 2, p)
    honest = pp.pack(up(pp, secrets), 7, seed=15)
    rows = honest.to_numpy().reshape(pp.n, 7, 4).copy()
    rows[3, 5] = rows[2, 1]
    sh = zk.DeviceBuffer.from_numpy(pp, rows)
    st = zk.DeviceBuffer(pp, 7)
    pp._check(pp.lib.zk_pss_repair(pp.h, sh.ptr, 7, 4, st.ptr, None, None, None))
    assert list(st.to_numpy(np.uint8)[:7]) == [0, 0, 0, 0, 0, 1, 0]
    assert np.array_equal(sh.to_numpy(), honest.to_numpy())
    for bad_k in (0, -1, pp.n, pp.n + 5):
        with pytest.raises(zk.ZkError) as e:
            pp.repair(sh, 7, bad_k)
        assert e.value.code == 4
    for args in ((None, st.ptr), (sh.ptr, None)):
        assert pp.lib.zk_pss_repair(pp.h, args[0], 7, 4, args[1], None, None, None) == 4
    # the context is still usable
    assert not pp.repair(sh, 7).status_host().any()
    assert pp.download_fr(pp.unpack(sh, 7)) == secrets
