"""The per-party entry points against the rank call they issue, world 1, eight host threads, one GPU, one
process, the method of tools/robust_bench.py: medians over R windows of B back-to-back calls with one stream synchronise
behind them, the calls of a row taking turns window by window.

usage: python tools/party_bench.py [--quick] [--reps R] [--batch B] [--out FILE]      -> ONE JSON line, also written to
       profiles/party_bench.json

Rows: d_fft at log2_m 15 and 20 (--quick: 15 only), BN254, l = 2, zero masks; then the SHA-256 proof (bench.py's circuit, all
twelve masks, no fixed-base tables in any column, since staged bases cannot use one).  Columns per row:
  rank        zk_dist_d_fft on the [8][m/l] block: the yardstick, measured in the same windows
  block       zk_party_d_fft from eight threads, rows carved from that block: zero copy, expected to differ by host time only
              (`block_minus_rank_us`)
  separate    zk_party_d_fft from eight threads, rows allocated one by one: one gather and one scatter launch around the call.
              Each reads and writes every staged byte once: 4 x 8 x (m/l) x 32 bytes of traffic per call, predicted at the
              6.29 TB/s copy figure of BASELINE.md (`staged_predicted_us`) beside what was measured (`staged_measured_us` =
              separate - block).
The proof row: zk_dist_groth16_prove against Party.prove on rows carved from the dealt [8][len] vectors and on separately
allocated rows; a proof call returns its shares, so the calls of a window follow each other without a synchronise.  Its staged
prediction is twice the bytes the gather launches moved (zk_party_stats), read once and written once, at the same figure."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zksaas_amd as zk
from zksaas_amd import net as znet
from zksaas_amd.api import DeviceBuffer, FftMask

COPY_TBS = 6.29


def raw(rng, count):
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


class Crew:
    """eight persistent threads; run(fn, batch) has thread i call fn(i) `batch` times, back to back, and returns when all have"""

    def __init__(self, k):
        self.k, self.job, self.errs = k, None, []
        self.start, self.end = threading.Barrier(k + 1), threading.Barrier(k + 1)
        self.threads = [threading.Thread(target=self._loop, args=(i,), daemon=True) for i in range(k)]
        for t in self.threads:
            t.start()

    def _loop(self, i):
        while True:
            self.start.wait()
            fn, batch = self.job
            try:
                for _ in range(batch):
                    fn(i)
            except BaseException as e:      # noqa: BLE001
                self.errs.append(e)
            self.end.wait()

    def run(self, fn, batch):
        self.job = (fn, batch)
        self.start.wait(timeout=120)
        self.end.wait(timeout=600)
        if self.errs:
            raise self.errs[0]


def proof_row(pp, net, parties, crew, a):
    from zksaas_amd import groth16 as zg
    from zksaas_amd import multigpu as mg
    from zksaas_amd import sha256_circuit as sc
    from zksaas_amd.fields import FR
    n, eb, p = pp.n, pp.fr.nbytes, FR["bn254"]
    r1, w = sc.build(1, 2, p, pad_wires=sc.REFERENCE_WIRES)
    rng = np.random.default_rng(42)
    td = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(5)]
    setup = zg.SetupScalars("bn254", r1, *td)
    crs = zg.Crs(pp, setup)
    wit = zg.Witness(pp, "bn254", r1, w, seed=43)
    r, s = (int.from_bytes(rng.bytes(32), "little") % p for _ in range(2))
    masks = zg.ProofMasks(pp, wit.log_m, seed=77)
    log_m, Lc = wit.log_m, (1 << wit.log_m) // pp.l
    e1, e2 = 2 * pp.fq.nbytes, 4 * pp.fq.nbytes
    lcrs = mg.LocalCrs(pp, crs, 0, n)
    qap, a_sh, ax_sh = mg.local_witness(pp, wit, 0, n)
    mct, keep = mg.local_masks(pp, masks, log_m, 0, n)
    # the device operands of a proof: (full [n][row] buffer, row bytes), in the order party_args reads them
    full = [(crs.s, crs.len_a * e1), (crs.h, crs.len_a * e1), (crs.v, crs.len_a * e2), (crs.w, crs.len_w * e1),
            (crs.u, crs.len_u * e1), (wit.qap[0], Lc * eb), (wit.qap[1], Lc * eb), (wit.qap[2], Lc * eb),
            (wit.a_share, wit.len_a * eb), (wit.ax_share, wit.len_w * eb)]
    full += [(m.in_mask, Lc * eb) for m in masks.fft] + [(m.out_mask, Lc * eb) for m in masks.fft]
    full += [(masks.degred.in_mask, Lc * eb), (masks.degred.out_mask, Lc * eb)]

    def carve(buf, row):
        return [buf.view(i * row, row) for i in range(n)]

    def separate(buf, row):
        host = buf.to_numpy(np.uint8).reshape(-1)[: n * row].reshape(n, row)
        out = []
        for i in range(n):
            b = DeviceBuffer(pp, row + 256)          # (the gap: never rows of one block)
            pp._check(pp.lib.zk_memcpy_h2d(pp.h, b.ptr, np.ascontiguousarray(host[i]).ctypes.data, row, None))
            out.append(b.view(0, row))
        return out

    s1, s2 = crs.s1, crs.s2
    keepalive = []

    def party_args(rows):
        """per party: (CrsShare, qap, a_share, ax_share, Masks) over its rows"""
        args = []
        for i in range(n):
            v = [op[i] for op in rows]
            ct = zg.CrsShare(v[0].ptr, v[1].ptr, v[2].ptr, v[3].ptr, v[4].ptr, crs.len_a, crs.len_w, crs.len_u,
                             s1[0].ctypes.data, s1[1].ctypes.data, s1[2].ctypes.data, s1[3].ctypes.data, s1[4].ctypes.data,
                             s2[0].ctypes.data, s2[1].ctypes.data, s2[2].ctypes.data)
            mk = zg.Masks()
            for j in range(6):
                mk.fft_in[j], mk.fft_out[j] = v[10 + j].ptr, v[16 + j].ptr
            mk.degred_in, mk.degred_out = v[22].ptr, v[23].ptr
            hm = []
            for j in range(5):
                x, y = np.ascontiguousarray(masks.msm[j].in_mask[i]), np.ascontiguousarray(masks.msm[j].out_mask[i])
                hm += [x, y]
                mk.msm_in[j], mk.msm_out[j] = x.ctypes.data, y.ctypes.data
            keepalive.append((v, hm))
            args.append((ct, [v[5], v[6], v[7]], v[8], v[9], mk))
        return args

    carved = party_args([carve(b, row) for b, row in full])
    sep = party_args([separate(b, row) for b, row in full])
    batch = max(1, a.batch // 4)

    def party_leg(args):
        return lambda: crew.run(lambda i: parties[i].prove(args[i][0], args[i][1], args[i][2], args[i][3], r, s, log_m,
                                                           masks=args[i][4], seed=9), batch)
    legs = [lambda: [znet.dist_prove(pp, net, lcrs.ct, qap, a_sh, ax_sh, r, s, log_m, masks=mct, seed=9) for _ in range(batch)],
            party_leg(carved), party_leg(sep)]
    for leg in legs:
        leg()
    pp.sync()
    ts = [[] for _ in legs]
    st = [None, None]
    for rep in range(a.reps):
        for j, leg in enumerate(legs):
            if j == 2 and rep == 0:
                st[0] = net.party_stats()
            t0 = time.perf_counter()
            leg()
            pp.sync()
            ts[j].append((time.perf_counter() - t0) / batch)
            if j == 2 and rep == 0:
                st[1] = net.party_stats()
    med = [sorted(t)[len(t) // 2] * 1e6 for t in ts]
    gathered = (st[1]["bytes_staged"] - st[0]["bytes_staged"]) // batch
    return {"call": "groth16_prove (SHA-256 circuit, all masks, no tables)", "log2_m": log_m, "rank_us": round(med[0], 2),
            "block_us": round(med[1], 2), "separate_us": round(med[2], 2), "block_minus_rank_us": round(med[1] - med[0], 2),
            "staged_traffic_bytes": 2 * gathered, "staged_predicted_us": round(2 * gathered / (COPY_TBS * 1e12) * 1e6, 2),
            "staged_measured_us": round(med[2] - med[1], 2), "batch": batch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "party_bench.json"))
    a = ap.parse_args()
    pp = zk.PackedSharingParams("bn254", 2)
    net = znet.StarNet(pp, 0, 1, None, "local", timeout_ms=5000)
    n, eb = pp.n, pp.fr.nbytes
    parties = [net.party(p) for p in range(n)]
    crew = Crew(n)
    rng = np.random.default_rng(1)
    rows_out = []
    for log_m in ([15] if a.quick else [15, 20]):
        Lc = (1 << log_m) // pp.l
        x = raw(rng, n * Lc).reshape(n, Lc * 4)
        block = DeviceBuffer.from_numpy(pp, x)
        carved = [block.view(i * Lc * eb, Lc * eb) for i in range(n)]
        sep = [DeviceBuffer(pp, Lc * eb + 256).view(0, Lc * eb) for _ in range(n)]       # (the gap: never rows of one block)
        for i, b in enumerate(sep):
            pp._check(pp.lib.zk_memcpy_h2d(pp.h, b.ptr, np.ascontiguousarray(x[i]).ctypes.data, Lc * eb, None))
        zero = FftMask.zero()
        legs = [
            lambda: [znet.dist_d_fft(pp, net, 0, block, zero, False, log_m, seed=3) for _ in range(a.batch)],
            lambda: crew.run(lambda i: parties[i].d_fft(0, carved[i], zero, False, log_m, seed=3), a.batch),
            lambda: crew.run(lambda i: parties[i].d_fft(0, sep[i], zero, False, log_m, seed=3), a.batch),
        ]
        for leg in legs:
            leg()
        pp.sync()
        st0 = net.party_stats()
        ts = [[] for _ in legs]
        for _ in range(a.reps):
            for j, leg in enumerate(legs):
                t0 = time.perf_counter()
                leg()
                pp.sync()
                ts[j].append((time.perf_counter() - t0) / a.batch)
        med = [sorted(t)[len(t) // 2] * 1e6 for t in ts]
        st1 = net.party_stats()
        staged_bytes = 4 * n * Lc * eb
        rows_out.append({
            "call": "d_fft", "log2_m": log_m, "rank_us": round(med[0], 2), "block_us": round(med[1], 2),
            "separate_us": round(med[2], 2), "block_minus_rank_us": round(med[1] - med[0], 2),
            "staged_traffic_bytes": staged_bytes, "staged_predicted_us": round(staged_bytes / (COPY_TBS * 1e12) * 1e6, 2),
            "staged_measured_us": round(med[2] - med[1], 2),
            "rounds": st1["rounds"] - st0["rounds"], "rounds_staged": st1["staged"] - st0["staged"]})
    if not a.quick:
        rows_out.append(proof_row(pp, net, parties, crew, a))
    out = {"tool": "party_bench", "curve": "bn254", "l": pp.l, "world": 1, "threads": n, "reps": a.reps, "batch": a.batch,
           "copy_tb_per_s": COPY_TBS, "rows": rows_out}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
