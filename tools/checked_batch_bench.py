"""The checked prover in batch and async form against the unchecked batch and against sequential checked proofs, on one GPU,
same process, same buffers, alternating -- DESIGN.md 4.11.9.  A record; no ratio is fixed in advance, one condition (below).

usage: python tools/checked_batch_bench.py [--quick] [--reps R] [--out FILE]      -> ONE JSON line

BN254, l = 2, the SHA-256 instance, all twelve masks per proof.  Rows (the calls of a row take turns window by window in one
process; a figure is the median over R windows of ONE call, host clock, the calls being synchronous -- tools/
checked_h_bench.py's method):
  batch        zk_groth16_prove_batch against zk_groth16_prove_checked_batch at nb = 4, 8, 16: clean, and with one lying
               party in one proof (its rows of qap_a / qap_b / qap_c of proof 1 random: the unchecked batch then computes a
               wrong proof 1 at the same cost, the checked one the honest proofs and a report that names the party)
  sequential   nb zk_groth16_prove_checked calls one after the other against ONE checked batch of nb, clean.
               `yardstick_spread_ms` is max - min of the sequential windows of the same run; `batch_not_slower` is
               batch <= sequential + that spread
  in_flight    two checked proofs in flight through zk_groth16_prove_checked_async (both started, then both joined) against
               the two in sequence"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zksaas_amd as zk
from zksaas_amd import groth16 as zg

L = 2
BAD = 3
SEED = 9


def windows(fns, reps):
    """median seconds per call of each fn, the fns taking turns window by window, and max - min per fn"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(time.perf_counter() - t0)
    return [sorted(t)[len(t) // 2] for t in ts], [max(t) - min(t) for t in ts]


def ms(t):
    return round(t * 1e3, 3)


def heads(pp, rep):
    return [s[:3] for s in rep.summaries]


def setting(pp, nmax):
    from zksaas_amd import sha256_circuit as sc
    from zksaas_amd.fields import FR
    p = FR["bn254"]
    r1, w = sc.build(1, 2, p, pad_wires=sc.REFERENCE_WIRES)
    rng = np.random.default_rng(42)
    td = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(5)]
    crs = zg.Crs(pp, zg.SetupScalars("bn254", r1, *td))
    wit = zg.Witness(pp, "bn254", r1, w, seed=43)
    rs = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(nmax)]
    ss = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(nmax)]
    masks = [zg.ProofMasks(pp, wit.log_m, seed=77 + 16 * b) for b in range(min(nmax, 4))]
    nch = (1 << wit.log_m) // L
    qap = []
    for k in range(3):
        rows = wit.qap[k].to_numpy().reshape(pp.n, nch, 4).copy()
        bad = rng.integers(0, 1 << 63, size=(nch, 4), dtype=np.uint64)
        bad[:, 3] &= np.uint64((1 << 60) - 1)
        rows[BAD] = bad
        qap.append(zk.DeviceBuffer.from_numpy(pp, rows))
    lying = types.SimpleNamespace(qap=qap, a_share=wit.a_share, ax_share=wit.ax_share, log_m=wit.log_m, len_a=wit.len_a,
                                  len_w=wit.len_w)
    return types.SimpleNamespace(crs=crs, wit=wit, lying=lying, rs=rs, ss=ss, masks=masks, nch=nch)


def batch_row(pp, S, nb, reps):
    mk = [S.masks[b % len(S.masks)] for b in range(nb)]
    res = {"nb": nb, "log2_m": S.wit.log_m}
    for leg in ("clean", "one_liar_in_proof_1"):
        wits = [S.wit] * nb if leg == "clean" else [S.wit, S.lying] + [S.wit] * (nb - 2)
        last = {}

        def unchecked():
            last["u"] = zg.prove_batch(pp, S.crs, wits, S.rs[:nb], S.ss[:nb], masks=mk, seed=SEED)

        def checked():
            last["c"] = zg.prove_batch(pp, S.crs, wits, S.rs[:nb], S.ss[:nb], masks=mk, seed=SEED, check=True)

        (tu, tc), _ = windows([unchecked, checked], reps)
        reports = last["c"][1]
        for b in range(nb):
            want = [[0, S.nch, 0]] * 3 + [[S.nch, 0, 0]] * 4 if leg != "clean" and b == 1 else [[S.nch, 0, 0]] * 7
            assert heads(pp, reports[b]) == want, (leg, b)
        res[leg] = {"unchecked_ms": ms(tu), "checked_ms": ms(tc), "ratio": round(tc / tu, 3),
                    "overhead_us_per_proof": round((tc - tu) * 1e6 / nb, 2), "checked_proofs_per_s": round(nb / tc, 1)}
    return res


def sequential_row(pp, S, nb, reps):
    mk = [S.masks[b % len(S.masks)] for b in range(nb)]
    last = {}

    def sequential():
        for b in range(nb):
            last["s"] = zg.prove(pp, S.crs, S.wit, S.rs[b], S.ss[b], masks=mk[b], seed=SEED + 16 * b, check=True)

    def batched():
        last["b"] = zg.prove_batch(pp, S.crs, [S.wit] * nb, S.rs[:nb], S.ss[:nb], masks=mk, seed=SEED, check=True)

    (ts, tb), (spread, _) = windows([sequential, batched], reps)
    assert heads(pp, last["s"][1]) == [[S.nch, 0, 0]] * 7
    assert all(heads(pp, r) == [[S.nch, 0, 0]] * 7 for r in last["b"][1])
    return {"nb": nb, "sequential_checked_ms": ms(ts), "checked_batch_ms": ms(tb), "ratio": round(tb / ts, 3),
            "yardstick_spread_ms": ms(spread), "batch_not_slower": bool(tb <= ts + spread)}


def in_flight_row(pp, S, reps):
    last = {}

    def one(b):
        return zg.prove_async(pp, S.crs, S.wit, S.rs[b], S.ss[b], masks=S.masks[b], seed=SEED + 16 * b, check=True)

    def sequential():
        for b in range(2):
            last["s"] = one(b).wait()

    def together():
        fl = [one(b) for b in range(2)]
        last["t"] = [f.wait() for f in fl]

    (ts, tt), (spread, _) = windows([sequential, together], reps)
    assert all(heads(pp, r) == [[S.nch, 0, 0]] * 7 for _, r in last["t"])
    return {"two_in_sequence_ms": ms(ts), "two_in_flight_ms": ms(tt), "ratio": round(tt / ts, 3),
            "yardstick_spread_ms": ms(spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    pp = zk.PackedSharingParams("bn254", L)
    sizes = [4] if a.quick else [4, 8, 16]
    S = setting(pp, max(sizes))
    out = {"tool": "checked_batch_bench", "curve": "bn254", "l": L, "reps": a.reps}
    out["batch"] = [batch_row(pp, S, nb, a.reps) for nb in sizes]
    out["sequential"] = [sequential_row(pp, S, nb, a.reps) for nb in sizes]
    out["in_flight"] = in_flight_row(pp, S, a.reps)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
