"""zk_pss_unpack against zk_pss_unpack_robust (the error-correcting unpack, csrc/gao.hpp) on one GPU, same process, same
buffers, alternating -- DESIGN.md 4.11.

usage: python tools/robust_bench.py [--quick] [--reps R] [--batch B] [--out FILE]      -> ONE JSON line

Shapes: BN254, l = 2 at 2^14 chunks (a vector of the SHA-256 proof) and 2^20 chunks, l = 8 at 2^20 chunks (--quick: 2^14 only).
Legs, each over shares of `pack` of random secrets, dimension 2l:
  clean        no share touched                      (stage 1 alone does the work; stage 2 finds an empty list and leaves)
  dirty_1pct   every 100th chunk has one wrong share (party 0)
  dirty_all    every chunk has one wrong share, the same party (3): what one bad rank does to a vector
Legs with a party list (zk_pss_unpack_robust_parties), at the same sizes:
  absent1_clean        the last party absent, the rest clean: against zk_pss_unpack2 with the same list (the dropout path)
  absent1_dirty_1pct   the last party absent, every 100th chunk with one wrong share (party 0) among the listed
  liar_listed_absent   the dirty_all vector with the lying party (3) listed absent: against zk_pss_unpack_robust on the
                       dirty_all vector itself, in turns (`ratio` = parties / dirty_all)
A figure is the median over R windows of B back-to-back calls with one stream synchronise behind them (host clock / B); the
two entry points take turns window by window.  `ratio` = robust / unpack.  `products_per_chunk` are the Fr products the code
executes per chunk, counted from the source: l n for unpack; for the clean path the inverse transform, the k l Horner steps
and the scalings (all SP lanes of a chunk); for a dirty chunk additionally n lanes times the products one lane of the decoder
executes with one error (interpolation n, 2 Euclid steps of 4, the inversion's 2, k division steps of 2, 2 k re-encoding).
With rho parties absent the clean path multiplies the n - rho listed shares at the load (every lane of a split loads them all)
and takes its Horner steps over k + rho coefficients; a dirty chunk's decoder runs at dimension k + rho and scales l secrets."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zksaas_amd as zk


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


def products(l, k):
    n, sp = 4 * l, 2 if l >= 8 else 1
    m = n // sp
    log_m = m.bit_length() - 1
    ifft = (m // 2) * (log_m - 1) - (m // 2 - 1)
    if sp == 1:
        horner = (k + 1) * l if l <= 2 else (k + 2) * l        # + the 1 / n; for l >= 4 + the walk of the point
        clean = ifft + horner
    else:
        clean = sp * ((m - 1) + ifft + l * (k // 2 + 4))         # the split's first stage; walk, square, X, 1 / n
    lane = n + 2 * 4 + 2 + 2 * k + 2 * k + 1
    return {"unpack": l * n, "robust_clean": clean, "decoder_per_dirty_chunk": n * lane}


def products_absent(l, k, rho):
    n, sp = 4 * l, 2 if l >= 8 else 1
    base, wide = products(l, k), products(l, k + rho)
    return {"unpack2": l * (n - rho), "robust_clean": wide["robust_clean"] + sp * (n - rho),
            "decoder_per_dirty_chunk": wide["decoder_per_dirty_chunk"] + (n - rho) + l,
            "robust_clean_all_parties": base["robust_clean"]}


def run_shape(l, log_chunks, reps, batch):
    pp = zk.PackedSharingParams("bn254", l)
    nch, n, k = 1 << log_chunks, 4 * l, 2 * l
    rng = np.random.default_rng(l * 100 + log_chunks)
    sec = zk.DeviceBuffer.from_numpy(pp, raw(rng, nch * l))
    shares = pp.pack(sec, nch, seed=1)
    out_u = pp.alloc_fr(l * nch)
    out_r = pp.alloc_fr(l * nch)
    status, errpos = zk.DeviceBuffer(pp, nch), zk.DeviceBuffer(pp, 4 * nch)
    summary = zk.DeviceBuffer(pp, 8 * (3 + n))
    lib, row = pp.lib, nch * pp.fr.nbytes

    def unpack():
        pp._check(lib.zk_pss_unpack(pp.h, shares.ptr, nch, out_u.ptr, None))

    def robust():
        pp._check(lib.zk_pss_unpack_robust(pp.h, shares.ptr, nch, k, out_r.ptr, None, status.ptr, errpos.ptr, summary.ptr, None))

    def set_row(party, arr):
        pp._check(lib.zk_memcpy_h2d(pp.h, shares.ptr + party * row, arr.ctypes.data, arr.nbytes, None))

    def get_row(party):
        arr = np.empty((nch, 4), dtype=np.uint64)
        pp._check(lib.zk_memcpy_d2h(pp.h, arr.ctypes.data, shares.ptr + party * row, arr.nbytes, None))
        return arr

    res = {"l": l, "log2_chunks": log_chunks, "dimension": k, "products_per_chunk": products(l, k)}
    want = sec.to_numpy()
    keep0, keep3 = get_row(0), get_row(3)
    for leg in ("clean", "dirty_1pct", "dirty_all"):
        if leg == "dirty_1pct":
            r0 = keep0.copy()
            r0[::100] = raw(rng, len(r0[::100]))
            set_row(0, r0)
        elif leg == "dirty_all":
            set_row(0, keep0)
            set_row(3, raw(rng, nch))
        tu, tr = windows(pp, [unpack, robust], reps, batch)
        s = [int(v) for v in summary.to_numpy(np.uint64)]
        ndirty = {"clean": 0, "dirty_1pct": len(keep0[::100]), "dirty_all": nch}[leg]
        assert s[:3] == [nch - ndirty, ndirty, 0], (leg, s)
        assert np.array_equal(out_r.to_numpy(), want), leg          # corrected: the original secrets
        res[leg] = {"unpack_us": round(tu * 1e6, 2), "robust_us": round(tr * 1e6, 2), "ratio": round(tr / tu, 3),
                    "robust_us_per_2p14_chunks": round(tr * 1e6 * (1 << 14) / nch, 2), "summary_head": s[:3]}
    # ---- the legs with a party list
    out_p = pp.alloc_fr(l * nch)

    def ids(parties):
        return (C.c_uint32 * len(parties))(*parties)

    def parties_call(buf, lst):
        arr = ids(lst)
        return lambda: pp._check(lib.zk_pss_unpack_robust_parties(pp.h, buf.ptr, arr, len(lst), nch, k, out_p.ptr, None,
                                                                  status.ptr, errpos.ptr, summary.ptr, None))

    # the lying party of dirty_all listed absent: its rows without row 3
    wo3 = [q for q in range(n) if q != 3]
    sh_wo3 = zk.DeviceBuffer(pp, (n - 1) * row)
    for i, q in enumerate(wo3):
        arr = get_row(q)
        pp._check(lib.zk_memcpy_h2d(pp.h, sh_wo3.ptr + i * row, arr.ctypes.data, arr.nbytes, None))
    t_all, t_abs = windows(pp, [robust, parties_call(sh_wo3, wo3)], reps, batch)
    s = [int(v) for v in summary.to_numpy(np.uint64)]
    assert s == [nch, 0, 0] + [0] * n, ("liar_listed_absent", s[:3])
    assert np.array_equal(out_p.to_numpy(), want), "liar_listed_absent"
    res["products_per_chunk_absent1"] = products_absent(l, k, 1)
    res["liar_listed_absent"] = {"robust_dirty_all_us": round(t_all * 1e6, 2), "robust_parties_us": round(t_abs * 1e6, 2),
                                 "ratio": round(t_abs / t_all, 4),
                                 "robust_parties_us_per_2p14_chunks": round(t_abs * 1e6 * (1 << 14) / nch, 2),
                                 "summary_head": s[:3]}
    del sh_wo3
    set_row(3, keep3)
    # the last party absent: the first n - 1 rows of the same buffer
    head = list(range(n - 1))
    head_ids = ids(head)

    def unpack2_head():
        pp._check(lib.zk_pss_unpack2(pp.h, shares.ptr, head_ids, n - 1, nch, out_u.ptr, None))

    for leg in ("absent1_clean", "absent1_dirty_1pct"):
        if leg == "absent1_dirty_1pct":
            set_row(0, r0)
        t2, tp = windows(pp, [unpack2_head, parties_call(shares, head)], reps, batch)
        s = [int(v) for v in summary.to_numpy(np.uint64)]
        ndirty = 0 if leg == "absent1_clean" else len(keep0[::100])
        assert s[:3] == [nch - ndirty, ndirty, 0] and s[3 + n - 1] == 0, (leg, s)
        assert np.array_equal(out_p.to_numpy(), want), leg
        res[leg] = {"unpack2_us": round(t2 * 1e6, 2), "robust_parties_us": round(tp * 1e6, 2), "ratio": round(tp / t2, 3),
                    "robust_parties_us_per_2p14_chunks": round(tp * 1e6 * (1 << 14) / nch, 2), "summary_head": s[:3]}
    set_row(0, keep0)
    pp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    shapes = [(2, 14)] if a.quick else [(2, 14), (2, 20), (8, 20)]
    out = {"tool": "robust_bench", "curve": "bn254", "reps": a.reps, "batch": a.batch,
           "shapes": [run_shape(l, lg, a.reps, a.batch) for l, lg in shapes]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
