"""The checked king rounds against the unchecked calls, and zk_pss_repair against zk_pss_unpack_robust, on one GPU, same
process, same buffers, alternating -- DESIGN.md 4.11.2.  A record for the decision on a king kernel fused with the scan; no
threshold.

usage: python tools/checked_king_bench.py [--quick] [--parties] [--reps R] [--batch B] [--out FILE]      -> ONE JSON line

BN254, l = 2.  Rows (the yardstick of each is the unchanged unchecked call in the same run):
  d_fft       zk_d_fft against zk_d_fft_checked at log2_m = 15 (the SHA-256 proof's) and 20, sampled masks, out of place:
              clean shares, and one lying party (its whole input row random; the unchecked call then computes garbage at the
              same cost, the checked one the honest output)
  repair      zk_pss_unpack_robust (secrets written) against zk_pss_repair at 2^14, 2^19 and 2^20 chunks: clean, and
              dirty_all (one lying party, every chunk dirty).  A repair leaves the word clean, so in the dirty leg BOTH calls
              are preceded by a device copy that puts the wrong row back; `restore_us` is that copy alone.
  deg_red     zk_deg_red against zk_deg_red_checked at 2^14 chunks, sampled masks, clean (in place: the output of a call
              is a clean input of the next)
  fixed       zk_pss_repair on 256 clean chunks, one workgroup of the scan: the per-call floor -- the clears of the count
              and of the summary, the scan's launch, and the stage-2 launch that finds an empty list
A figure is the median over R windows of B back-to-back calls with one stream synchronise behind them (host clock / B); the
two entry points take turns window by window (tools/robust_bench.py's method).  `scan_products_per_chunk` is counted from the
source (gao_ifft: 1 / 5 / 17 at l = 1, 2, 4).  `scan_share_of_clean_overhead` = (repair_clean - fixed) / (checked - unchecked)
at the same number of chunks: the part of the clean-path overhead that is the scan's pass over the matrix, which is what a
king kernel fused with the scan could remove at most (it would still execute the scan's products).

--parties: the rows of DESIGN.md 4.11.3 instead -- the calls with a party list, every yardstick in the same windows:
  d_fft_parties   at log2_m = 15 and 20, five calls taking turns: zk_d_fft (unchecked), zk_d_fft_checked on clean shares and
              on the one-lying-party vector (the rows above, measured again), and zk_d_fft_checked_parties as
              `liar_left_out` (the one-lying-party vector, that party absent) and `one_absent_clean` (honest shares, the last
              party absent).  Ratios are against the unchecked call.
  repair_parties  zk_pss_repair_parties alone at 2^14, 2^19 and 2^20 chunks on the compact rows: `absent1_clean` (honest
              shares, the last party absent) and `liar_listed_absent` (the one-lying-party vector without that party's row),
              against zk_pss_repair on the same vectors: clean, and dirty (every chunk reaches the decoder; preceded by the
              device copy that puts the wrong row back, `restore_us` is that copy alone)
  d_pp        zk_d_pp against zk_d_pp_checked on clean shares at 2^14 and 2^20 chunks, sampled masks (both calls end with
              the host's read of the zero-denominator flag)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zksaas_amd as zk

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
    return round(t * 1e6, 2)


def tensor(arr):
    """a device tensor of int64 limbs (the library's calls take its data_ptr; both use the null stream)"""
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def report(pp, nch):
    return zk.DeviceBuffer(pp, nch), zk.DeviceBuffer(pp, 4 * nch), zk.DeviceBuffer(pp, 8 * (3 + pp.n))


def summary_of(buf):
    return [int(v) for v in buf.to_numpy(np.uint64)]


def honest(pp, nch, rng, seed):
    return pp.pack(zk.DeviceBuffer.from_numpy(pp, raw(rng, nch * L)), nch, seed=seed).to_numpy().reshape(pp.n, nch, 4)


def d_fft_row(pp, log_m, reps, batch):
    n, nch = pp.n, (1 << log_m) // L
    rng = np.random.default_rng(log_m)
    rows = honest(pp, nch, rng, 1)
    mask = zk.FftMask.sample(pp, False, None, False, log_m, 2)
    out_u, out_c = pp.alloc_fr(n * nch), pp.alloc_fr(n * nch)
    status, errpos, summary = report(pp, nch)
    res = {"log2_m": log_m, "chunks": nch}
    want = None
    for leg in ("clean", "one_liar"):
        if leg == "one_liar":
            rows = rows.copy()
            rows[BAD] = raw(rng, nch)
        x = zk.DeviceBuffer.from_numpy(pp, rows)

        def unchecked():
            pp._check(pp.lib.zk_d_fft(pp.h, x.ptr, mask.in_mask.ptr, mask.out_mask.ptr, 0, log_m, 7, out_u.ptr, None))

        def checked():
            pp._check(pp.lib.zk_d_fft_checked(pp.h, x.ptr, mask.in_mask.ptr, mask.out_mask.ptr, 0, log_m, 7, out_c.ptr,
                                              status.ptr, errpos.ptr, summary.ptr, None))

        tu, tc = windows(pp, [unchecked, checked], reps, batch)
        s = summary_of(summary)
        if leg == "clean":      # (the shares' randomness is the production stream: outputs are compared as secrets)
            want = pp.unpack(out_u, nch).to_numpy().copy()
            assert s[:3] == [nch, 0, 0], s
        else:
            assert s[:3] == [0, nch, 0] and s[3 + BAD] == nch, s
        assert np.array_equal(pp.unpack(out_c, nch).to_numpy(), want), leg            # the honest output
        res[leg] = {"unchecked_us": us(tu), "checked_us": us(tc), "ratio": round(tc / tu, 3), "overhead_us": us(tc - tu),
                    "summary_head": s[:3]}
    return res


def repair_row(pp, log_chunks, reps, batch):
    n, nch, k = pp.n, 1 << log_chunks, 2 * L
    rng = np.random.default_rng(100 + log_chunks)
    rows = honest(pp, nch, rng, 3)
    sh = tensor(rows)
    wrong = tensor(raw(rng, nch))
    sec = pp.alloc_fr(L * nch)
    status, errpos, summary = report(pp, nch)
    p = sh.data_ptr()

    def robust():
        pp._check(pp.lib.zk_pss_unpack_robust(pp.h, p, nch, k, sec.ptr, None, status.ptr, errpos.ptr, summary.ptr, None))

    def repair():
        pp._check(pp.lib.zk_pss_repair(pp.h, p, nch, k, status.ptr, errpos.ptr, summary.ptr, None))

    def restore():
        sh[BAD].copy_(wrong)

    res = {"log2_chunks": log_chunks, "scan_products_per_chunk": {1: 1, 2: 5, 4: 17}[L]}
    tr, tp = windows(pp, [robust, repair], reps, batch)
    assert summary_of(summary)[:3] == [nch, 0, 0]
    res["clean"] = {"robust_us": us(tr), "repair_us": us(tp), "ratio": round(tp / tr, 3)}
    t0, tr, tp = windows(pp, [restore, lambda: (restore(), robust()), lambda: (restore(), repair())], reps, batch)
    s = summary_of(summary)
    assert s[:3] == [0, nch, 0] and s[3 + BAD] == nch, s
    assert np.array_equal(sh.cpu().numpy().view(np.uint64), rows)      # repaired: the honest matrix
    res["dirty_all"] = {"restore_us": us(t0), "robust_us": us(tr), "repair_us": us(tp), "ratio": round(tp / tr, 3),
                        "ratio_without_restore": round((tp - t0) / (tr - t0), 3)}
    return res


def deg_red_row(pp, log_chunks, reps, batch):
    n, nch = pp.n, 1 << log_chunks
    rng = np.random.default_rng(200 + log_chunks)
    mask = zk.DegRedMask.sample(pp, nch, 4)
    xu = zk.DeviceBuffer.from_numpy(pp, honest(pp, nch, rng, 5))
    xc = zk.DeviceBuffer.from_numpy(pp, xu.to_numpy())
    status, errpos, summary = report(pp, nch)

    def unchecked():
        pp._check(pp.lib.zk_deg_red(pp.h, xu.ptr, mask.in_mask.ptr, mask.out_mask.ptr, nch, 9, None))

    def checked():
        pp._check(pp.lib.zk_deg_red_checked(pp.h, xc.ptr, mask.in_mask.ptr, mask.out_mask.ptr, nch, 9, status.ptr, errpos.ptr,
                                            summary.ptr, None))

    tu, tc = windows(pp, [unchecked, checked], reps, batch)
    assert summary_of(summary)[:3] == [nch, 0, 0]
    assert np.array_equal(pp.unpack(xu, nch).to_numpy(), pp.unpack(xc, nch).to_numpy())      # the same secrets
    return {"log2_chunks": log_chunks, "clean": {"unchecked_us": us(tu), "checked_us": us(tc), "ratio": round(tc / tu, 3),
                                                  "overhead_us": us(tc - tu)}}


def fixed_row(pp, reps, batch):
    nch = 256
    sh = zk.DeviceBuffer.from_numpy(pp, honest(pp, nch, np.random.default_rng(300), 6))
    status, errpos, summary = report(pp, nch)
    (t,) = windows(pp, [lambda: pp._check(pp.lib.zk_pss_repair(pp.h, sh.ptr, nch, 2 * L, status.ptr, errpos.ptr, summary.ptr,
                                                                None))], reps, batch)
    return {"chunks": nch, "repair_us": us(t), "what": "two clears, the scan's launch, the stage-2 launch that finds an empty list"}


def d_fft_parties_row(pp, log_m, reps, batch):
    import ctypes as C
    n, nch = pp.n, (1 << log_m) // L
    rng = np.random.default_rng(log_m)
    rows = honest(pp, nch, rng, 1)
    lying = rows.copy()
    lying[BAD] = raw(rng, nch)
    mask = zk.FftMask.sample(pp, False, None, False, log_m, 2)
    x, y = zk.DeviceBuffer.from_numpy(pp, rows), zk.DeviceBuffer.from_numpy(pp, lying)
    outs = [pp.alloc_fr(n * nch) for _ in range(5)]
    reps_ = [report(pp, nch) for _ in range(4)]
    no_liar = [q for q in range(n) if q != BAD]
    no_last = list(range(n - 1))
    ids_liar, ids_last = (C.c_uint32 * (n - 1))(*no_liar), (C.c_uint32 * (n - 1))(*no_last)

    def unchecked():
        pp._check(pp.lib.zk_d_fft(pp.h, x.ptr, mask.in_mask.ptr, mask.out_mask.ptr, 0, log_m, 7, outs[0].ptr, None))

    def checked(src, i):
        st, ep, sm = reps_[i]
        return lambda: pp._check(pp.lib.zk_d_fft_checked(pp.h, src.ptr, mask.in_mask.ptr, mask.out_mask.ptr, 0, log_m, 7,
                                                         outs[1 + i].ptr, st.ptr, ep.ptr, sm.ptr, None))

    def listed(src, ids, i):
        st, ep, sm = reps_[i]
        return lambda: pp._check(pp.lib.zk_d_fft_checked_parties(pp.h, src.ptr, ids, n - 1, mask.in_mask.ptr,
                                                                 mask.out_mask.ptr, 0, log_m, 7, outs[1 + i].ptr, st.ptr,
                                                                 ep.ptr, sm.ptr, None))

    names = ["checked_clean", "checked_one_liar", "liar_left_out", "one_absent_clean"]
    fns = [unchecked, checked(x, 0), checked(y, 1), listed(y, ids_liar, 2), listed(x, ids_last, 3)]
    ts = windows(pp, fns, reps, batch)
    want = pp.unpack(outs[0], nch).to_numpy().copy()
    heads = [summary_of(r[2]) for r in reps_]
    assert heads[0][:3] == [nch, 0, 0] and heads[1][:3] == [0, nch, 0] and heads[1][3 + BAD] == nch, heads[:2]
    assert heads[2] == [nch, 0, 0] + [0] * n and heads[3] == [nch, 0, 0] + [0] * n, heads[2:]      # nothing reached stage 2
    for o in outs[1:]:
        assert np.array_equal(pp.unpack(o, nch).to_numpy(), want)                                  # the honest output
    res = {"log2_m": log_m, "chunks": nch, "unchecked_us": us(ts[0])}
    for name, t, h in zip(names, ts[1:], heads):
        res[name] = {"us": us(t), "ratio_to_unchecked": round(t / ts[0], 3), "overhead_us": us(t - ts[0]), "summary_head": h[:3]}
    res["liar_left_out"]["ratio_to_checked_one_liar"] = round(ts[3] / ts[2], 3)
    return res


def repair_parties_row(pp, log_chunks, reps, batch):
    import ctypes as C
    n, nch, k = pp.n, 1 << log_chunks, 2 * L
    rng = np.random.default_rng(100 + log_chunks)
    rows = honest(pp, nch, rng, 3)
    wrong_rows = raw(rng, nch)
    lying = rows.copy()
    lying[BAD] = wrong_rows
    no_liar = [q for q in range(n) if q != BAD]
    clean_all, dirty_all = tensor(rows), tensor(lying)
    wrong = tensor(wrong_rows)
    no_last_rows, no_liar_rows = tensor(rows[:n - 1]), tensor(lying[no_liar])
    ids_last, ids_liar = (C.c_uint32 * (n - 1))(*range(n - 1)), (C.c_uint32 * (n - 1))(*no_liar)
    r = [report(pp, nch) for _ in range(4)]

    def repair(buf, i):
        return lambda: pp._check(pp.lib.zk_pss_repair(pp.h, buf.data_ptr(), nch, k, r[i][0].ptr, r[i][1].ptr, r[i][2].ptr,
                                                      None))

    def listed(buf, ids, i):
        return lambda: pp._check(pp.lib.zk_pss_repair_parties(pp.h, buf.data_ptr(), ids, n - 1, nch, k, r[i][0].ptr,
                                                              r[i][1].ptr, r[i][2].ptr, None))

    def restore():
        dirty_all[BAD].copy_(wrong)

    dirty = repair(dirty_all, 1)
    ts = windows(pp, [repair(clean_all, 0), restore, lambda: (restore(), dirty()), listed(no_last_rows, ids_last, 2),
                      listed(no_liar_rows, ids_liar, 3)], reps, batch)
    heads = [summary_of(x[2]) for x in r]
    assert heads[0][:3] == [nch, 0, 0] and heads[1][:3] == [0, nch, 0] and heads[1][3 + BAD] == nch, heads[:2]
    assert heads[2] == [nch, 0, 0] + [0] * n and heads[3] == [nch, 0, 0] + [0] * n, heads[2:]
    return {"log2_chunks": log_chunks,
            "repair_clean_us": us(ts[0]), "restore_us": us(ts[1]), "repair_dirty_with_restore_us": us(ts[2]),
            "repair_dirty_us": us(ts[2] - ts[1]),
            "absent1_clean": {"us": us(ts[3]), "ratio_to_repair_clean": round(ts[3] / ts[0], 3)},
            "liar_listed_absent": {"us": us(ts[4]), "ratio_to_repair_clean": round(ts[4] / ts[0], 3),
                                   "ratio_to_repair_dirty": round(ts[4] / (ts[2] - ts[1]), 3)}}


def d_pp_row(pp, log_chunks, reps, batch):
    n, nch = pp.n, 1 << log_chunks
    rng = np.random.default_rng(400 + log_chunks)
    num, den = (zk.DeviceBuffer.from_numpy(pp, honest(pp, nch, rng, 10 + i)) for i in range(2))
    mask = zk.DegRedMask.sample(pp, nch, 12)
    out_u, out_c = pp.alloc_fr(n * nch), pp.alloc_fr(n * nch)
    status, errpos = zk.DeviceBuffer(pp, 2 * nch), zk.DeviceBuffer(pp, 8 * nch)
    summary = zk.DeviceBuffer(pp, 16 * (3 + n))

    def unchecked():
        pp._check(pp.lib.zk_d_pp(pp.h, num.ptr, den.ptr, mask.in_mask.ptr, mask.out_mask.ptr, nch, 13, out_u.ptr, None))

    def checked():
        pp._check(pp.lib.zk_d_pp_checked(pp.h, num.ptr, den.ptr, None, n, mask.in_mask.ptr, mask.out_mask.ptr, nch, 13,
                                         out_c.ptr, status.ptr, errpos.ptr, summary.ptr, None))

    tu, tc = windows(pp, [unchecked, checked], reps, batch)
    s = summary_of(summary)
    assert s[:3] == [nch, 0, 0] and s[3 + n:6 + n] == [nch, 0, 0], s
    assert np.array_equal(pp.unpack(out_u, nch).to_numpy(), pp.unpack(out_c, nch).to_numpy())      # the same secrets
    return {"log2_chunks": log_chunks, "clean": {"unchecked_us": us(tu), "checked_us": us(tc), "ratio": round(tc / tu, 3),
                                                  "overhead_us": us(tc - tu)}}


def main_all_parties(pp, a):
    out = {"tool": "checked_king_bench", "curve": "bn254", "l": L, "reps": a.reps, "batch": a.batch}
    out["fixed"] = fixed_row(pp, a.reps, a.batch)
    out["d_fft"] = [d_fft_row(pp, lg, a.reps, a.batch) for lg in ([15] if a.quick else [15, 20])]
    out["repair"] = [repair_row(pp, lg, a.reps, a.batch) for lg in ([14] if a.quick else [14, 19, 20])]
    out["deg_red"] = [deg_red_row(pp, 14, a.reps, a.batch)]
    by_chunks = {r["log2_chunks"]: r for r in out["repair"]}
    for row in out["d_fft"]:
        rep = by_chunks.get(row["log2_m"] - 1)
        if rep and row["clean"]["overhead_us"] > 0:
            scan = rep["clean"]["repair_us"] - out["fixed"]["repair_us"]
            row["scan_share_of_clean_overhead"] = round(scan / row["clean"]["overhead_us"], 3)
    return out


def main_parties(pp, a):
    out = {"tool": "checked_king_bench --parties", "curve": "bn254", "l": L, "reps": a.reps, "batch": a.batch}
    out["d_fft_parties"] = [d_fft_parties_row(pp, lg, a.reps, a.batch) for lg in ([15] if a.quick else [15, 20])]
    out["repair_parties"] = [repair_parties_row(pp, lg, a.reps, a.batch) for lg in ([14] if a.quick else [14, 19, 20])]
    out["d_pp"] = [d_pp_row(pp, lg, a.reps, a.batch) for lg in ([14] if a.quick else [14, 20])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--parties", action="store_true", help="the rows with a party list (DESIGN.md 4.11.3)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    pp = zk.PackedSharingParams("bn254", L)
    if a.parties:
        out = main_parties(pp, a)
    else:
        out = main_all_parties(pp, a)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
