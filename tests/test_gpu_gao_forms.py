"""GPU test (through the C ABI): ONE host driver and ONE kernel pair serve every form of the repair of packed scalar shares.
The same dirty matrix [n][nchunks] goes through the five public forms that can take it,
  zk_pss_repair,  zk_pss_repair_parties with all n listed,  zk_pss_repair_batch with one item,
  zk_pss_repair_batch_parties with one item and all n listed,  zk_pss_repair_range over the whole word
  (stride = cnt = len, base = shift = 0),
and all five must leave identical shares, status, errpos and summary, byte for byte; then its compact matrix of a list of
n - 1 parties goes through the three forms that take a list, which must agree in the same way.  Both are also compared with
tests/gao_erasure_model.py, which is asked first, on the CPU, about every generated chunk: each one is clean or corrected,
none is beyond the cap, so nothing is left out of the comparison.
  shapes   nchunks in {1, 65, 700}: one lane, a partial second wave, and three workgroups of stage 1 with the last one partial
           (at l = 8, where a chunk takes two lanes, six workgroups of 128 chunks)
  words    dimension 2l, one wrong share in about a tenth of the chunks (chunk 0 always, so the single chunk is dirty), a
           fixed seed.  With n - 1 parties listed the cap is l - 1: at l = 1 a listed wrong share could only be detected, so
           there every wrong share is the absent party's and the compact matrix is clean.
The matrix and the model's verdicts are computed once per (curve, l) at 700 chunks; the smaller shapes are its first columns."""
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

CONFIGS = [(c, l) for c in ("bn254", "bls12_381") for l in (1, 2, 4, 8)]
IDS = ["%s_l%d" % c for c in CONFIGS]
SIZES = [1, 65, 700]
NCH = max(SIZES)


def _absent(l):
    return 2 * l                       # the party the list of n - 1 leaves out


def _decoded(words, S, k, w, p):
    """the model's verdict on every chunk, and the matrix it would leave -> (status, errpos, rows after the repair)"""
    status, errpos, fixed = [], [], [list(r) for r in words]
    for c in range(len(words[0])):
        d = em.decode([r[c] for r in words], S, k, w, p)
        status.append(d.status)
        errpos.append(d.errpos)
        if d.status == 1:
            for i, q in enumerate(S):
                if (d.errpos >> q) & 1:
                    fixed[i][c] = gm.poly_eval(d.message, pow(w, q, p), p)
    return status, errpos, fixed


@functools.lru_cache(maxsize=None)
def _data(curve, l):
    """the dirty matrix as limbs [n][NCH][nl] and, for all n parties and for the list of n - 1, the model's
    (parties, status, errpos, repaired rows as limbs).  Computed once and never changed: the callers copy."""
    pp, o = ctx(curve, l), opp(curve, l)
    p, w = o.p, o.share.group_gen
    n, k, e = 4 * l, 2 * l, _absent(l)
    rnd = random.Random(20240 + l)
    xs = [pow(w, q, p) for q in range(n)]
    rows = [[0] * NCH for _ in range(n)]
    liars = [e] if l == 1 else list(range(n))
    for c in range(NCH):
        msg = [rnd.randrange(p) for _ in range(k)]
        for q in range(n):
            rows[q][c] = gm.poly_eval(msg, xs[q], p)
        if c == 0 or rnd.random() < 0.1:
            q = rnd.choice(liars) if c or l == 1 else 1         # (chunk 0: a listed party wherever the list can correct)
            rows[q][c] = (rows[q][c] + rnd.randrange(1, p)) % p
    enc = lambda m: np.stack([pp.fr.encode(r) for r in m])
    out = {"rows": enc(rows)}
    for name, S in (("all", list(range(n))), ("list", [q for q in range(n) if q != e])):
        status, errpos, fixed = _decoded([rows[q] for q in S], S, k, w, p)
        # asked on the CPU before anything runs: every chunk is clean or corrected, none beyond the cap
        assert set(status) <= {0, 1} and status[0] == (0 if (name, l) == ("list", 1) else 1), (curve, l, name)
        assert all(bin(ep).count("1") == st for st, ep in zip(status, errpos)), (curve, l, name)
        out[name] = (S, np.array(status, np.uint8), np.array(errpos, np.uint32), enc(fixed))
    assert 40 <= int(out["all"][1].sum()) <= 110           # about a tenth of the chunks
    assert l == 1 or int(out["list"][1].sum()) >= 30
    return out


def _dev(pp, arr):
    return zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(arr))


def _report(r):
    return r.out.to_numpy(np.uint8), r.status_host(), r.errpos_host(), r.summary


def _range(pp, m, parties, nch, dim):
    """zk_pss_repair_range over the whole word -> the same four outputs"""
    buf = _dev(pp, m)
    status, errpos = zk.DeviceBuffer(pp, nch), zk.DeviceBuffer(pp, 4 * nch)
    summary = _dev(pp, np.full(3 + pp.n, 77, np.uint64))
    arr = None if parties is None else (C.c_uint32 * len(parties))(*parties)
    pp._check(pp.lib.zk_pss_repair_range(pp.h, buf.ptr, arr, m.shape[0], nch, nch, nch, 0, 0, dim, status.ptr, errpos.ptr,
                                         summary.ptr, None))
    pp.sync()
    return (buf.to_numpy(np.uint8), status.to_numpy(np.uint8), errpos.to_numpy(np.uint32),
            [int(v) for v in summary.to_numpy(np.uint64)])


def _batch_of_one(pp, m, parties, nch, dim):
    r = pp.repair_batch(_dev(pp, m), 1, nch, dim, parties=parties)
    assert len(r.summaries) == 1
    return _report(r)


def _agree(pp, forms, model, nch, what):
    """every form's outputs are the first form's, byte for byte, and the model's"""
    S, status, errpos, fixed = model
    status, errpos, fixed = status[:nch], errpos[:nch], np.ascontiguousarray(fixed[:, :nch])
    summary = [int((status == s).sum()) for s in (0, 1, 2)] + [int(((errpos >> q) & 1).sum()) for q in range(pp.n)]
    name0, first = forms[0]
    assert np.array_equal(first[0], fixed.view(np.uint8).reshape(-1)), (what, name0)
    assert np.array_equal(first[1], status) and np.array_equal(first[2], errpos) and first[3] == summary, (what, name0)
    for name, got in forms[1:]:
        assert got[0].tobytes() == first[0].tobytes(), (what, name, "shares")
        assert got[1].tobytes() == first[1].tobytes(), (what, name, "status")
        assert got[2].tobytes() == first[2].tobytes(), (what, name, "errpos")
        assert got[3] == first[3], (what, name, "summary")


@pytest.mark.parametrize("nch", SIZES)
@pytest.mark.parametrize("curve,l", CONFIGS, ids=IDS)
def test_every_form_of_the_repair_is_the_same_call(curve, l, nch):
    pp = ctx(curve, l)
    n, dim = pp.n, 2 * l
    data = _data(curve, l)
    m = np.ascontiguousarray(data["rows"][:, :nch])
    full = list(range(n))
    _agree(pp, [("repair", _report(pp.repair(_dev(pp, m), nch, dim))),
                ("repair_parties", _report(pp.repair(_dev(pp, m), nch, dim, parties=full))),
                ("repair_batch", _batch_of_one(pp, m, None, nch, dim)),
                ("repair_batch_parties", _batch_of_one(pp, m, full, nch, dim)),
                ("repair_range", _range(pp, m, None, nch, dim))], data["all"], nch, (curve, l, nch, "all n"))
    S = data["list"][0]
    ms = np.ascontiguousarray(m[S])
    _agree(pp, [("repair_parties", _report(pp.repair(_dev(pp, ms), nch, dim, parties=S))),
                ("repair_batch_parties", _batch_of_one(pp, ms, S, nch, dim)),
                ("repair_range", _range(pp, ms, S, nch, dim))], data["list"], nch, (curve, l, nch, "n - 1"))
