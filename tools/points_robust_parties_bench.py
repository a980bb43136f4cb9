"""zk_pss_unpack_points_robust_parties against the calls it stands next to, and zk_groth16_reconstruct_robust against
zk_groth16_reconstruct, one proof at a time.

Method as tools/points_robust_bench.py: medians of windows, the calls of a row taking turns window by window in one process.
BN254, l = 2 (n = 8), dimension 2l, G1 and G2, 2^10 and 2^14 chunks.
  all_listed   the party form with nparties == n against zk_pss_unpack_points_robust on the same clean shares.  EXPECTATION:
               the same cost, within the spread (min .. max) of the all-party call's own windows in this run: the kernels are
               the same text, the syndrome scalars come from the list's table instead of the packing factor's
  one_absent   party 5 absent, clean shares, against zk_pss_unpack2_points with the same list: 3 syndrome rows + 2 secret rows
               of 7 inputs against 2 rows of 7
  one_liar     the same list with party 3 lying in every chunk: the scan, then stage 2 on every chunk
  reconstruct  zk_groth16_reconstruct_robust over nproofs synthetic proofs (shares of dimension 2l lifted to points, Z = 1)
               against nproofs calls of zk_groth16_reconstruct (host Straus), at 1, 16, 256 and 4096 proofs
Writes one JSON line (and --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zksaas_amd as zk
from zksaas_amd.api import ZK_G1, ZK_G2
from points_robust_bench import lift, raw, summary_of, us

L = 2
BAD, GONE = 3, 5


def windows(pp, fns, reps, batch, sync=True):
    """(median, min, max) seconds per call of each fn, the fns taking turns window by window"""
    for fn in fns:
        fn()
    pp.sync()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(batch):
                fn()
            if sync:
                pp.sync()
            ts[i].append((time.perf_counter() - t0) / batch)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def unpack_row(pp, group, log_chunks, reps, batch):
    n, nch, k = pp.n, 1 << log_chunks, 2 * L
    rng = np.random.default_rng(800 + log_chunks)
    rows = pp.pack(zk.DeviceBuffer.from_numpy(pp, raw(rng, nch * L)), nch, seed=41).to_numpy().reshape(n, nch, 4)
    lying = rows.copy()
    lying[BAD] = raw(rng, nch)
    S = [q for q in range(n) if q != GONE]
    ids_all, ids = (C.c_uint32 * n)(*range(n)), (C.c_uint32 * len(S))(*S)
    clean = lift(pp, group, zk.DeviceBuffer.from_numpy(pp, rows), n * nch).reshape(n, nch, -1)
    sub_clean = lift(pp, group, zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(rows[S])), len(S) * nch)
    sub_liar = lift(pp, group, zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(lying[S])), len(S) * nch)
    w = clean.shape[2]
    outs = [torch.zeros((nch * L, w), dtype=torch.int64, device="cuda") for _ in range(5)]
    rep = [(zk.DeviceBuffer(pp, nch), zk.DeviceBuffer(pp, 4 * nch), zk.DeviceBuffer(pp, 8 * (3 + n))) for _ in range(4)]

    def all_party():
        st, ep, sm = rep[0]
        pp._check(pp.lib.zk_pss_unpack_points_robust(pp.h, group, clean.data_ptr(), nch, k, outs[0].data_ptr(), st.ptr, ep.ptr,
                                                     sm.ptr, None))

    def listed(src, arr, cnt, i):
        st, ep, sm = rep[i]
        return lambda: pp._check(pp.lib.zk_pss_unpack_points_robust_parties(pp.h, group, src.data_ptr(), arr, cnt, nch, k,
                                                                            outs[i].data_ptr(), st.ptr, ep.ptr, sm.ptr, None))

    def plain2():
        pp._check(pp.lib.zk_pss_unpack2_points(pp.h, group, sub_clean.data_ptr(), ids, len(S), nch, outs[4].data_ptr(), None))

    ts = windows(pp, [all_party, listed(clean, ids_all, n, 1), plain2, listed(sub_clean, ids, len(S), 2),
                      listed(sub_liar, ids, len(S), 3)], reps, batch)
    heads = [summary_of(r[2]) for r in rep]
    assert heads[0][:3] == [nch, 0, 0] and heads[1] == heads[0] and heads[2] == heads[0], heads
    assert heads[3][:3] == [0, nch, 0] and heads[3][3 + BAD] == nch, heads
    for o in outs[1:]:
        assert torch.equal(o, outs[0])                       # the honest secrets, byte for byte
    (t_all, lo, hi), (t_lst, _, _), (t_p2, _, _), (t_abs, _, _), (t_liar, _, _) = ts
    return {"group": "G2" if group == ZK_G2 else "G1", "log2_chunks": log_chunks,
            "all_listed": {"all_party_us": us(t_all), "all_party_min_us": us(lo), "all_party_max_us": us(hi), "us": us(t_lst),
                           "ratio": round(t_lst / t_all, 3), "within_spread": bool(lo <= t_lst <= hi)},
            "unpack2_points_us": us(t_p2),
            "one_absent": {"us": us(t_abs), "ratio": round(t_abs / t_p2, 3), "rows_expected": (L + len(S) - k) / L},
            "one_liar": {"us": us(t_liar), "ratio": round(t_liar / t_p2, 3), "stage2_us": us(t_liar - t_abs)}}


def reconstruct_row(pp, nproofs, reps):
    n, nl = pp.n, pp.fq.nl
    rng = np.random.default_rng(900 + nproofs)
    one = pp.fq.encode([1]).reshape(-1)

    def shares(group, seed):
        rows = pp.pack(zk.DeviceBuffer.from_numpy(pp, raw(rng, nproofs * L)), nproofs, seed=seed)
        aff = lift(pp, group, rows, n * nproofs).cpu().numpy().view(np.uint64).reshape(n, nproofs, -1)
        z = np.zeros((n, nproofs, aff.shape[2] // 2), dtype=np.uint64)
        z[:, :, :nl] = one
        return np.ascontiguousarray(np.concatenate([aff, z], axis=2).transpose(1, 0, 2))        # [nproofs][n] Jacobian

    pa, pb, pc = shares(ZK_G1, 51), shares(ZK_G2, 52), shares(ZK_G1, 53)
    aff = np.zeros((nproofs, 8 * nl), dtype=np.uint64)
    by = np.zeros((nproofs, 4 * pp.fq.nbytes), dtype=np.uint8)
    aff1, by1 = np.zeros_like(aff), np.zeros_like(by)
    st = np.full((nproofs, 3), 255, dtype=np.uint8)

    def robust():
        pp._check(pp.lib.zk_groth16_reconstruct_robust(pp.h, nproofs, pa.ctypes.data, pb.ctypes.data, pc.ctypes.data, None, n,
                                                       aff.ctypes.data, by.ctypes.data, st.ctypes.data, None, None))

    def one_by_one():
        for i in range(nproofs):
            pp._check(pp.lib.zk_groth16_reconstruct(pp.h, pa[i].ctypes.data, pb[i].ctypes.data, pc[i].ctypes.data, None, n,
                                                    aff1[i].ctypes.data, by1[i].ctypes.data, None))

    (t_r, _, _), (t_1, _, _) = windows(pp, [robust, one_by_one], reps, 1, sync=False)        # both calls are synchronous
    assert not st.any() and np.array_equal(aff, aff1) and np.array_equal(by, by1)
    return {"nproofs": nproofs, "robust_us": us(t_r), "reconstruct_calls_us": us(t_1), "ratio": round(t_r / t_1, 3),
            "robust_us_per_proof": us(t_r / nproofs), "reconstruct_us_per_proof": us(t_1 / nproofs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    pp = zk.PackedSharingParams("bn254", L)
    out = {"tool": "points_robust_parties_bench", "curve": "bn254", "l": L, "reps": a.reps, "batch": a.batch}
    out["unpack"] = [unpack_row(pp, g, lg, a.reps, a.batch) for g in (ZK_G1, ZK_G2) for lg in ([10] if a.quick else [10, 14])]
    out["reconstruct"] = [reconstruct_row(pp, m, 3 if m >= 4096 else a.reps) for m in ([1, 16] if a.quick else [1, 16, 256, 4096])]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
