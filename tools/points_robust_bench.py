"""zk_pss_unpack_points_robust and zk_pss_repair_points against the unchanged zk_pss_unpack_points, and zk_d_msm_checked against
zk_d_msm, on one GPU, same process, same buffers, alternating -- DESIGN.md 4.11.4.  A record; no threshold.

usage: python tools/points_robust_bench.py [--quick] [--reps R] [--batch B] [--out FILE]      -> ONE JSON line

BN254, l = 2 (n = 8, dimension 4), G1 and G2.  Rows at 2^10 and 2^14 chunks; the yardstick of each is zk_pss_unpack_points of
the same windows:
  clean       the robust unpack on honest shares: l + (n - k) = 6 rows of n-input double-and-add where the unpack walks l = 2
  one_liar    the robust unpack with one party's whole row wrong: the same 6 rows, then stage 2 on every chunk -- per chunk one
              product per lane for the location (n lanes), one round of n lanes for the two consistency checks and the l output
              products, and l affine conversions
  repair      zk_pss_repair_points alone on the one-liar vector: n - k = 4 rows, then stage 2 with one output.  A repair leaves
              the word clean, so the call is preceded by a device copy that puts the wrong row back; `restore_us` is that
              copy alone and is subtracted
  repair_clean  zk_pss_repair_points on honest shares: the 4 syndrome rows and nothing else
  d_msm       zk_d_msm against zk_d_msm_checked at len 2^16 with sampled masks: two fused MSMs where the unchecked call runs one
A figure is the median over R windows of B back-to-back calls with one stream synchronise behind them (host clock / B); the
calls of a row take turns window by window (tools/checked_king_bench.py's method).  `rows_expected` next to a ratio is the
count of double-and-add rows per chunk relative to the unpack's l."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zksaas_amd as zk
from zksaas_amd.api import ZK_G1, ZK_G2
from zksaas_amd.groth16 import G1_GEN, G2_GEN

L = 2
BAD = 3


def raw(rng, count):
    """random field elements as Montgomery limbs: anything below 2^252 is below every scalar modulus here"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def windows(pp, fns, reps, batch):
    """median seconds per call of each fn, the fns taking turns window by window"""
    for fn in fns:
        fn()
    pp.sync()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(batch):
                fn()
            pp.sync()
            ts[i].append((time.perf_counter() - t0) / batch)
    return [sorted(t)[len(t) // 2] for t in ts]


def us(t):
    return round(t * 1e6, 1)


def gen_limbs(pp, group):
    g = G2_GEN["bn254"] if group == ZK_G2 else G1_GEN["bn254"]
    flat = [g[0][0], g[0][1], g[1][0], g[1][1]] if group == ZK_G2 else list(g)
    return np.ascontiguousarray(pp.fq.encode(flat).reshape(-1))


def lift(pp, group, scalars_d, count):
    """device scalars -> a torch tensor of affine points s G (int64 limbs)"""
    w = pp.fq.nl * (4 if group == ZK_G2 else 2)
    out = torch.zeros((count, w), dtype=torch.int64, device="cuda")
    gen = gen_limbs(pp, group)
    pp._check(pp.lib.zk_base_mul(pp.h, group, gen.ctypes.data, scalars_d.ptr, count, out.data_ptr(), None))
    pp.sync()
    return out


def summary_of(buf):
    return [int(v) for v in buf.to_numpy(np.uint64)]


def unpack_row(pp, group, log_chunks, reps, batch):
    n, nch, k = pp.n, 1 << log_chunks, 2 * L
    rng = np.random.default_rng(500 + log_chunks)
    rows = pp.pack(zk.DeviceBuffer.from_numpy(pp, raw(rng, nch * L)), nch, seed=31).to_numpy().reshape(n, nch, 4)
    lying = rows.copy()
    lying[BAD] = raw(rng, nch)
    clean = lift(pp, group, zk.DeviceBuffer.from_numpy(pp, rows), n * nch).reshape(n, nch, -1)
    dirty = lift(pp, group, zk.DeviceBuffer.from_numpy(pp, lying), n * nch).reshape(n, nch, -1)
    wrong = dirty[BAD].clone()
    work = dirty.clone()                   # what the repair writes
    w = clean.shape[2]
    outs = [torch.zeros((nch * L, w), dtype=torch.int64, device="cuda") for _ in range(3)]
    rep = [(zk.DeviceBuffer(pp, nch), zk.DeviceBuffer(pp, 4 * nch), zk.DeviceBuffer(pp, 8 * (3 + n))) for _ in range(4)]

    def plain():
        pp._check(pp.lib.zk_pss_unpack_points(pp.h, group, clean.data_ptr(), nch, outs[0].data_ptr(), None))

    def robust(src, i):
        st, ep, sm = rep[i]
        return lambda: pp._check(pp.lib.zk_pss_unpack_points_robust(pp.h, group, src.data_ptr(), nch, k, outs[1 + i].data_ptr(),
                                                                    st.ptr, ep.ptr, sm.ptr, None))

    def repair(src, i):
        st, ep, sm = rep[i]
        return lambda: pp._check(pp.lib.zk_pss_repair_points(pp.h, group, src.data_ptr(), nch, k, st.ptr, ep.ptr, sm.ptr, None))

    def restore():
        work[BAD].copy_(wrong)

    fix = repair(work, 2)
    ts = windows(pp, [plain, robust(clean, 0), robust(dirty, 1), restore, lambda: (restore(), fix()), repair(clean, 3)],
                 reps, batch)
    heads = [summary_of(r[2]) for r in rep]
    assert heads[0][:3] == [nch, 0, 0] and heads[3][:3] == [nch, 0, 0], heads
    assert heads[1][:3] == [0, nch, 0] and heads[1][3 + BAD] == nch and heads[2] == heads[1], heads
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])          # the honest secrets, byte for byte
    assert torch.equal(work, clean)                                                 # repaired: the honest matrix
    t_plain, t_clean, t_liar, t_restore, t_fix, t_scan = ts
    nsyn = n - k
    return {"group": "G2" if group == ZK_G2 else "G1", "log2_chunks": log_chunks, "unpack_points_us": us(t_plain),
            "clean": {"us": us(t_clean), "ratio": round(t_clean / t_plain, 3), "rows_expected": (L + nsyn) / L},
            "one_liar": {"us": us(t_liar), "ratio": round(t_liar / t_plain, 3), "ratio_to_clean": round(t_liar / t_clean, 3),
                         "rows_expected": (L + nsyn) / L, "stage2_us": us(t_liar - t_clean)},
            "repair": {"restore_us": us(t_restore), "us": us(t_fix - t_restore), "ratio": round((t_fix - t_restore) / t_plain, 3),
                       "rows_expected": nsyn / L},
            "repair_clean": {"us": us(t_scan), "ratio": round(t_scan / t_plain, 3), "rows_expected": nsyn / L}}


def d_msm_row(pp, group, log_len, reps, batch):
    n, ln = pp.n, 1 << log_len
    rng = np.random.default_rng(600 + log_len)
    bases = lift(pp, group, pp.det_pack(zk.DeviceBuffer.from_numpy(pp, raw(rng, ln * L)), ln), n * ln)
    scal = pp.pack(zk.DeviceBuffer.from_numpy(pp, raw(rng, ln * L)), ln, seed=32)
    mask = zk.MsmMask.sample(pp, group, gen_limbs(pp, group), 33)
    nl = pp.fq.nl * (2 if group == ZK_G2 else 1)
    out_u, out_c = np.zeros((n, 3 * nl), dtype=np.uint64), np.zeros((n, 3 * nl), dtype=np.uint64)
    status = C.c_uint8(255)
    im, om = mask.in_mask.ctypes.data, mask.out_mask.ctypes.data

    def unchecked():
        pp._check(pp.lib.zk_d_msm(pp.h, group, bases.data_ptr(), scal.ptr, ln, im, om, out_u.ctypes.data, None))

    def checked():
        pp._check(pp.lib.zk_d_msm_checked(pp.h, group, bases.data_ptr(), scal.ptr, ln, im, om, out_c.ctypes.data,
                                          C.addressof(status), None))

    tu, tc = windows(pp, [unchecked, checked], reps, batch)
    assert status.value == 0          # (Jacobian outputs are not canonical: two zk_d_msm calls differ in their bytes too)
    return {"group": "G2" if group == ZK_G2 else "G1", "log2_len": log_len, "d_msm_us": us(tu), "d_msm_checked_us": us(tc),
            "ratio": round(tc / tu, 3), "msms_expected": 2.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    pp = zk.PackedSharingParams("bn254", L)
    out = {"tool": "points_robust_bench", "curve": "bn254", "l": L, "reps": a.reps, "batch": a.batch}
    out["unpack"] = [unpack_row(pp, g, lg, a.reps, a.batch) for g in (ZK_G1, ZK_G2) for lg in ([10] if a.quick else [10, 14])]
    out["d_msm"] = [d_msm_row(pp, g, 12 if a.quick else 16, a.reps, a.batch) for g in (ZK_G1, ZK_G2)]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
