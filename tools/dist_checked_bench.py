"""zk_dist_d_fft against zk_dist_d_fft_checked (the checked king round on the star network, engine_dist.inc.hpp) over the
shared-memory transport, all ranks on one GPU, the two calls taking turns in ONE set of processes -- DESIGN.md 4.11.7.

usage: python tools/dist_checked_bench.py [--log-m 20] [--world 8] [--reps 5] [--batch 2] [--out FILE]      -> ONE JSON line

Per king mode (star, all-to-all) and leg:
  honest     packed shares of random secrets: the scan alone does the work
  liar_1pct  rank 3 lies in every 100th chunk: the king's word is fft1(x) + in_mask, formed on the rank, so rank 3 passes an
             in-mask row that is nonzero in those chunks (every other rank a row of zeros, so that all ranks issue the same
             launches); those chunks reach the decoder and are corrected
  liar_all   rank 3's whole vector replaced before every call: every chunk reaches the decoder and is corrected
Three calls take turns: zk_dist_d_fft, zk_dist_d_fft_checked, and zk_dist_d_fft_checked with summary_d == NULL, which runs the
repair and skips the summary's collective -- `nosummary_us` separates the two parts of the added time.
Method of tools/robust_bench.py: a figure is the median over R windows of B back-to-back calls with one stream synchronise
behind them (host clock / B, on rank 0, which hosts the star king); the calls of a row take turns window by window.  Every
call is preceded by the same device copy of the rank's pristine rows into the work buffer (the round runs in place), timed
alone as `copy_us` and subtracted from neither figure."""
import argparse
import json
import multiprocessing as mp
import os
import queue
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(rank, world, net_id, log_m, reps, batch, q):
    try:
        import zksaas_amd as zk
        from zksaas_amd import net as znet
        from zksaas_amd.api import DeviceBuffer
        # every rank deals the whole sharing itself and keeps its rows: the dealing must be the same on every rank, so the
        # contexts run on the replayable share randomness (a rank's own production stream would give each a sharing of its own)
        zk.api.DEFAULT_OPTIONS["rng_replay"] = 1
        pp = zk.PackedSharingParams("bn254", 2)
        net = znet.StarNet(pp, rank, world, net_id, "shm", timeout_ms=120000)
        n, l, k = pp.n, pp.l, net.k
        Lc = (1 << log_m) // l
        rng = np.random.default_rng(1)            # the same dealing on every rank

        def raw(count):
            a = rng.integers(0, 1 << 62, size=(count, 4), dtype=np.uint64)
            a[:, 3] &= np.uint64((1 << 60) - 1)
            return a

        shares = pp.pack(DeviceBuffer.from_numpy(pp, raw(Lc * l)), Lc, seed=1).to_numpy().reshape(n, Lc, 4)
        junk = raw(Lc)
        rows = {"honest": np.ascontiguousarray(shares[net.parties])}
        bad = shares.copy()
        bad[3] = junk
        rows["liar_all"] = np.ascontiguousarray(bad[net.parties])
        rows["liar_1pct"] = rows["honest"]
        del shares, bad
        # the in-mask rows of this rank: zeros, but for party 3 a nonzero element in every 100th chunk
        mrows = np.zeros((n, Lc, 4), np.uint64)
        mrows[3, ::100] = junk[::100]
        ndirty = len(range(0, Lc, 100))
        mask1 = DeviceBuffer.from_numpy(pp, np.ascontiguousarray(mrows[net.parties]))
        del mrows
        work = pp.alloc_fr(k * Lc)
        nbytes = k * Lc * pp.fr.nbytes
        zero = pp.alloc_fr(k * Lc)
        zeros_host = np.zeros(nbytes, np.uint8)        # (held in a name: the copy reads it)
        pp._check(pp.lib.zk_memcpy_h2d(pp.h, zero.ptr, zeros_host.ctypes.data, nbytes, None))
        del zeros_host
        status, errpos = DeviceBuffer(pp, Lc), DeviceBuffer(pp, 4 * Lc)
        summary = DeviceBuffer(pp, 8 * (3 + n))
        res = {}
        if rank == 0:
            print("dist_checked_bench: %d ranks dealt 2^%d" % (world, log_m), file=sys.stderr, flush=True)
        for mode in ("star", "alltoall"):
            pp.set_option("king_alltoall", int(mode == "alltoall"))
            for leg in ("honest", "liar_1pct", "liar_all"):
                src = DeviceBuffer.from_numpy(pp, rows[leg])
                im = mask1.ptr if leg == "liar_1pct" else None

                def reset():       # work = src: zero the buffer's rows through vec_mul_sub(out = a * b - c) with b = 0, c = -src
                    pp._check(pp.lib.zk_vec_mul_sub(pp.h, work.ptr, zero.ptr, zero.ptr, neg.ptr, k * Lc, None))

                neg = pp.alloc_fr(k * Lc)          # -src, made once: 0 * 0 - src
                pp._check(pp.lib.zk_vec_mul_sub(pp.h, neg.ptr, zero.ptr, zero.ptr, src.ptr, k * Lc, None))

                def plain():
                    reset()
                    pp._check(pp.lib.zk_dist_d_fft(pp.h, net.h, 0, work.ptr, im, None, 0, log_m, 3, None))

                def checked():
                    reset()
                    pp._check(pp.lib.zk_dist_d_fft_checked(pp.h, net.h, 0, work.ptr, im, None, 0, log_m, 3, status.ptr,
                                                           errpos.ptr, summary.ptr, None))

                def nosummary():
                    reset()
                    pp._check(pp.lib.zk_dist_d_fft_checked(pp.h, net.h, 0, work.ptr, im, None, 0, log_m, 3, status.ptr,
                                                           errpos.ptr, None, None))

                fns = [plain, checked, nosummary]
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
                tu, tc, tn = [sorted(t)[len(t) // 2] for t in ts]
                t0 = time.perf_counter()
                for _ in range(batch):
                    reset()
                pp.sync()
                tcopy = (time.perf_counter() - t0) / batch
                s = [int(v) for v in summary.to_numpy(np.uint64)]
                nd = {"honest": 0, "liar_1pct": ndirty, "liar_all": Lc}[leg]
                want = [Lc - nd, nd, 0] + [nd if p == 3 else 0 for p in range(n)]
                assert s == want, (mode, leg, s[:6])
                res["%s_%s" % (mode, leg)] = {"unchecked_us": round(tu * 1e6, 1), "checked_us": round(tc * 1e6, 1),
                                              "added_us": round((tc - tu) * 1e6, 1), "ratio": round(tc / tu, 3),
                                              "nosummary_us": round(tn * 1e6, 1), "nosummary_added_us": round((tn - tu) * 1e6, 1),
                                              "copy_us": round(tcopy * 1e6, 1), "summary_head": s[:3]}
                if rank == 0:              # progress, leg by leg (a run of this size is minutes long)
                    print("dist_checked_bench: %s_%s %r" % (mode, leg, res["%s_%s" % (mode, leg)]), file=sys.stderr, flush=True)
                del src, neg
            st = net.stats()
            res[mode + "_alltoalls"] = st["alltoalls"]
        q.put((rank, True, res))
        net.close()
    except Exception as e:      # noqa: BLE001
        import traceback
        q.put((rank, False, traceback.format_exc()[-2000:] + repr(e)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-m", type=int, default=20)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--limit", type=float, default=900.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    from zksaas_amd.net import StarNet
    net_id = StarNet.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, a.world, net_id, a.log_m, a.reps, a.batch, q)) for r in range(a.world)]
    for p in procs:
        p.start()
    results, deadline = [], time.monotonic() + a.limit
    try:
        while len(results) < a.world:
            try:
                results.append(q.get(timeout=2.0))
            except queue.Empty:
                died = [(i, p.exitcode) for i, p in enumerate(procs) if p.exitcode not in (None, 0)]
                if died or time.monotonic() > deadline:      # a rank that is gone leaves the others waiting for it: end them
                    print("dist_checked_bench: no result from every rank (died: %r)" % died, file=sys.stderr, flush=True)
                    sys.exit(1)
    finally:
        for p in procs:
            p.join(timeout=30 if len(results) == a.world else 0)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
            if p.is_alive():               # a rank stuck in a device wait does not outlive the tool
                p.kill()
                p.join(timeout=10)
    bad = [r for r in results if not r[1]]
    if bad:
        print(bad, file=sys.stderr)
        sys.exit(1)
    by_rank = {r[0]: r[2] for r in results}
    out = {"tool": "dist_checked_bench", "curve": "bn254", "l": 2, "log2_m": a.log_m, "world": a.world, "transport": "shm",
           "reps": a.reps, "batch": a.batch, "rank0": by_rank[0],
           "added_us_by_rank": {key: [by_rank[r][key]["added_us"] for r in range(a.world)]
                                for key in by_rank[0] if isinstance(by_rank[0][key], dict)}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
