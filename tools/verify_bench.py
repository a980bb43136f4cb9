"""The verifier timed on one GPU: us per proof of zk_groth16_verify and of zk_groth16_verify_all (one verdict for the batch)
and us per pairing of zk_multi_pairing (k = 1) at count = 1, 16, 256, 4096, 16384 and 65536 on BN254 and BLS12-381.
usage: python tools/verify_bench.py [--counts 1,16,...] [--curves bn254,bls12_381] [--reps 7] [--out FILE] [--cpu-oracle]
                                    [--alternate] [--bytes] [--subgroup]
--bytes alternates zk_groth16_verify (points as given, no subgroup test) with zk_groth16_verify_bytes (decode, subgroup test
and pairing check from the wire bytes) on the same proofs, rep by rep, and prints per count what the checked call adds and how
much of that the new kernels' own slot times account for: the rest is host time or a stall.  --subgroup times
zk_points_subgroup_check per group: points per second.
--alternate times only the two verifier calls, interleaved rep by rep in one process (per-proof, batch, per-proof, ...) on
arrays encoded once outside the timed region, so that both see the same clocks and the same neighbours: the yardstick for
"from which count does the batch call win".  Call a count faster only where the two min-max ranges do not overlap.
Per (curve, call, count): one warm-up call, then `reps` timed calls (host clock around a call that returns with the
result on the host or in device memory after its own wait), reported as median, min and max; the per-kernel share comes
from the library's HIP-event slots (pairing_miller_kernel, pairing_final_exp_kernel) over the same calls.  The proofs are
real ones of a small circuit (one public input), repeated to fill the batch; every verdict is checked.  Spread between
machines is not measured by one run: run it on two and state both.  --cpu-oracle also times the Python oracle's
verify_proof on this machine's CPU (the only verifier the project had before), one proof.
A kernel profile of the same calls: rocprofv3 --kernel-trace --stats -d DIR -- python tools/verify_bench.py --reps 2"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zksaas_amd as zk
from zksaas_amd import groth16 as zg
from zksaas_amd.api import ZK_G1, ZK_G2, multi_pairing


def small_r1cs(P, nc=11):
    """a chain of nc multiplication gates with one public output"""
    from zksaas_amd.sha256_circuit import R1CS
    w = [1, 0, 7, 5]
    A, B, Cm = [], [], []
    for _ in range(nc - 1):
        k = len(w)
        w.append((w[k - 1] + 3) * (w[k - 1] + w[k - 2]) % P)
        A.append([(1, k - 1), (3, 0)])
        B.append([(1, k - 1), (1, k - 2)])
        Cm.append([(1, k)])
    A.append([(1, len(w) - 1)])
    B.append([(1, 0)])
    Cm.append([(1, 1)])
    w[1] = w[-1]
    return R1CS(2, len(w) - 2, A, B, Cm), w


def slots(pp):
    out = {}
    for slot in range(pp.lib.zk_profile_slots()):
        name = pp.lib.zk_profile_name(slot).decode()
        if not name.startswith(("pairing_", "points_subgroup", "points_decompress_checked", "verify_")):
            continue
        ms, units, calls = C.c_double(), C.c_double(), C.c_long()
        pp._check(pp.lib.zk_profile_read(pp.h, slot, C.byref(ms), C.byref(units), C.byref(calls)))
        if calls.value:
            out[name] = round(ms.value / calls.value * 1e3, 1)          # us per launch
    return out


def timed(pp, fn, reps):
    fn()                                                              # warm-up: code objects, allocations
    pp._check(pp.lib.zk_profile_enable(pp.h, 1))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    k = slots(pp)
    pp._check(pp.lib.zk_profile_enable(pp.h, 0))
    return ts, k


def run(curve, counts, reps):
    pp = zk.PackedSharingParams(curve, 2)
    P = zk.fields.FR[curve]
    r1, w = small_r1cs(P)
    setup = zg.SetupScalars(curve, r1, 11, 12, 13, 14, 15)
    crs = zg.Crs(pp, setup)
    wit = zg.Witness(pp, curve, r1, w, seed=5)
    aff, _ = zg.reconstruct(pp, zg.prove(pp, crs, wit, 21, 22, seed=9), want_bytes=False)
    vk = zg.verifying_key(pp, setup)
    pvk = zg.PreparedVk(pp, vk)
    rows = []
    for count in counts:
        proofs = np.tile(aff, (count, 1))
        xs = [[w[1]]] * count
        res = []
        ts, k = timed(pp, lambda: res.append(zg.verify(pp, pvk, proofs, xs)), reps)
        assert all(all(r) for r in res), "a valid proof was rejected"
        rows.append(row(curve, "zk_groth16_verify", count, ts, k))
        res = []
        ts, k = timed(pp, lambda: res.append(zg.verify_all(pp, pvk, proofs, xs)), reps)
        assert all(res), "a valid batch was rejected"
        rows.append(row(curve, "zk_groth16_verify_all", count, ts, k))
        sc = pp.upload_fr([3 + i for i in range(count)])
        p1, q2 = zg.base_points(pp, ZK_G1, sc, count), zg.base_points(pp, ZK_G2, sc, count)
        out = zk.DeviceBuffer(pp, count * 12 * pp.fq.nbytes)
        ts, k = timed(pp, lambda: multi_pairing(pp, p1, q2, 1, count, out=out), reps)
        rows.append(row(curve, "zk_multi_pairing k=1", count, ts, k))
        for b in (sc, p1, q2, out):
            b.free()
    return rows, (pp, vk, aff, w)


def run_alternate(curve, counts, reps):
    """zk_groth16_verify and zk_groth16_verify_all through the C ABI on the same host arrays, one warm-up each, then `reps`
    rounds of (per-proof call, batch call); the kernel slots are read in a profiled round of their own after the timed ones"""
    pp = zk.PackedSharingParams(curve, 2)
    P = zk.fields.FR[curve]
    r1, w = small_r1cs(P)
    setup = zg.SetupScalars(curve, r1, 11, 12, 13, 14, 15)
    aff, _ = zg.reconstruct(pp, zg.prove(pp, zg.Crs(pp, setup), zg.Witness(pp, curve, r1, w, seed=5), 21, 22, seed=9),
                            want_bytes=False)
    pvk = zg.PreparedVk(pp, zg.verifying_key(pp, setup))
    rows = []
    for count in counts:
        proofs = np.ascontiguousarray(np.tile(np.asarray(aff, dtype=np.uint64).reshape(1, -1), (count, 1)))
        xs = np.ascontiguousarray(np.tile(pp.fr.encode([w[1]]).reshape(1, -1), (count, 1)))
        ok = np.zeros(count, dtype=np.uint8)
        allok = C.c_int(0)

        def each():
            pp._check(pp.lib.zk_groth16_verify(pp.h, pvk.h, proofs.ctypes.data, xs.ctypes.data, 1, count, ok.ctypes.data, None))
            assert ok.all(), "a valid proof was rejected"

        def batch():
            pp._check(pp.lib.zk_groth16_verify_all(pp.h, pvk.h, proofs.ctypes.data, xs.ctypes.data, 1, count, None,
                                                   C.byref(allok), None, None))
            assert allok.value == 1, "a valid batch was rejected"

        each()
        batch()
        t = {"zk_groth16_verify": [], "zk_groth16_verify_all": []}
        for _ in range(reps):
            for name, fn in (("zk_groth16_verify", each), ("zk_groth16_verify_all", batch)):
                t0 = time.perf_counter()
                fn()
                t[name].append(time.perf_counter() - t0)
        for name, fn in (("zk_groth16_verify", each), ("zk_groth16_verify_all", batch)):
            pp._check(pp.lib.zk_profile_enable(pp.h, 1))
            fn()
            k = slots(pp)
            pp._check(pp.lib.zk_profile_enable(pp.h, 0))
            rows.append(row(curve, name + " (alternating)", count, t[name], k))
        a, b = t["zk_groth16_verify"], t["zk_groth16_verify_all"]
        verdict = "batch faster" if max(b) < min(a) else "per-proof faster" if max(a) < min(b) else "ranges overlap"
        print(json.dumps({"curve": curve, "count": count, "verdict": verdict,
                          "ratio_of_medians": round(statistics.median(a) / statistics.median(b), 2)}), flush=True)
    return rows


NEW_KERNELS = ("verify_stage_points_kernel", "verify_stage_inputs_kernel", "verify_valid_and_kernel")


def run_bytes(curve, counts, reps):
    """zk_groth16_verify on the affine points and zk_groth16_verify_bytes on the wire bytes of the same proofs, one warm-up
    each, then `reps` rounds of (unchecked, bytes); the kernel slots are read in a profiled round of their own"""
    pp = zk.PackedSharingParams(curve, 2)
    P = zk.fields.FR[curve]
    r1, w = small_r1cs(P)
    setup = zg.SetupScalars(curve, r1, 11, 12, 13, 14, 15)
    aff, raw = zg.reconstruct(pp, zg.prove(pp, zg.Crs(pp, setup), zg.Witness(pp, curve, r1, w, seed=5), 21, 22, seed=9))
    pvk = zg.PreparedVk(pp, zg.verifying_key(pp, setup))
    rows = []
    for count in counts:
        proofs = np.ascontiguousarray(np.tile(np.asarray(aff, dtype=np.uint64).reshape(1, -1), (count, 1)))
        xs = np.ascontiguousarray(np.tile(pp.fr.encode([w[1]]).reshape(1, -1), (count, 1)))
        pb = np.ascontiguousarray(np.tile(np.frombuffer(raw, dtype=np.uint8), count))
        xb = np.ascontiguousarray(np.tile(np.frombuffer(int(w[1]).to_bytes(32, "little"), dtype=np.uint8), count))
        ok = np.zeros(count, dtype=np.uint8)

        def plain():
            pp._check(pp.lib.zk_groth16_verify(pp.h, pvk.h, proofs.ctypes.data, xs.ctypes.data, 1, count, ok.ctypes.data, None))
            assert ok.all(), "a valid proof was rejected"

        def checked():
            pp._check(pp.lib.zk_groth16_verify_bytes(pp.h, pvk.h, pb.ctypes.data, xb.ctypes.data, 1, count, ok.ctypes.data, None))
            assert ok.all(), "a valid proof was rejected"

        calls = (("zk_groth16_verify", plain), ("zk_groth16_verify_bytes", checked))
        plain()
        checked()
        t = {name: [] for name, _ in calls}
        for _ in range(reps):
            for name, fn in calls:
                t0 = time.perf_counter()
                fn()
                t[name].append(time.perf_counter() - t0)
        ks = {}
        for name, fn in calls:
            pp._check(pp.lib.zk_profile_enable(pp.h, 1))
            fn()
            ks[name] = slots(pp)
            pp._check(pp.lib.zk_profile_enable(pp.h, 0))
            rows.append(row(curve, name + " (alternating)", count, t[name], ks[name]))
        a, b = statistics.median(t["zk_groth16_verify"]), statistics.median(t["zk_groth16_verify_bytes"])
        new_ms = sum(ks["zk_groth16_verify_bytes"].get(k, 0.0) for k in NEW_KERNELS) / 1e3
        acc = {"curve": curve, "count": count, "extra_ms": round((b - a) * 1e3, 3), "new_kernels_ms": round(new_ms, 3),
               "unaccounted_ms": round((b - a) * 1e3 - new_ms, 3),
               "unaccounted_share_of_the_call": round(((b - a) * 1e3 - new_ms) / (b * 1e3), 4)}
        print(json.dumps(acc), flush=True)
        rows.append(acc)
    return rows


def run_subgroup(curve, counts, reps):
    """zk_points_subgroup_check on `count` random multiples of the generator, per group: points per second"""
    pp = zk.PackedSharingParams(curve, 2)
    rows = []
    for count in counts:
        sc = pp.upload_fr([3 + 5 * i for i in range(count)])
        for group, name in ((ZK_G1, "G1"), (ZK_G2, "G2")):
            pts = zg.base_points(pp, group, sc, count)
            okd = zk.DeviceBuffer(pp, count)

            def check():
                pp._check(pp.lib.zk_points_subgroup_check(pp.h, group, pts.ptr, count, okd.ptr, None))

            ts, k = timed(pp, check, reps)
            assert okd.to_numpy(dtype=np.uint8)[:count].all(), "a subgroup point was rejected"
            r = row(curve, "zk_points_subgroup_check " + name, count, ts, k)
            r["points_per_s"] = round(count / statistics.median(ts))
            rows.append(r)
            pts.free()
            okd.free()
        sc.free()
    return rows


def row(curve, call, count, ts, kernels):
    med = statistics.median(ts)
    r = {"curve": curve, "call": call, "count": count, "reps": len(ts), "median_ms": round(med * 1e3, 3),
         "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3), "us_per_item": round(med / count * 1e6, 2),
         "kernels_us_per_launch": kernels}
    print(json.dumps(r), flush=True)
    return r


def cpu_oracle(curve, pp, vk, aff, w):
    from oracle import pairing as op
    from oracle.curve import g1
    from oracle.params import CURVES
    c = CURVES[curve]
    v = pp.fq.decode(np.asarray(aff).reshape(-1, pp.fq.nl))
    proof = ((v[0], v[1]), ((v[2], v[3]), (v[4], v[5])), (v[6], v[7]))
    ovk = op.VerifyingKey(vk["alpha_g1"], vk["beta_g2"], vk["gamma_g2"], vk["delta_g2"], vk["gamma_abc_g1"])
    t0 = time.perf_counter()
    ok = op.verify_proof(c, ovk, proof, [w[1]], g1(c))
    return {"curve": curve, "call": "oracle.pairing.verify_proof (CPU, Python ints)", "count": 1, "ok": ok,
            "us_per_item": round((time.perf_counter() - t0) * 1e6, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,16,256,4096,16384,65536")
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu-oracle", action="store_true")
    ap.add_argument("--alternate", action="store_true")
    ap.add_argument("--bytes", action="store_true")
    ap.add_argument("--subgroup", action="store_true")
    a = ap.parse_args()
    mode = " --alternate" if a.alternate else " --bytes" if a.bytes else " --subgroup" if a.subgroup else ""
    out = {"tool": "tools/verify_bench.py" + mode, "reps": a.reps, "rows": []}
    for curve in a.curves.split(","):
        if a.bytes or a.subgroup:
            out["rows"] += (run_bytes if a.bytes else run_subgroup)(curve, [int(c) for c in a.counts.split(",")], a.reps)
            continue
        if a.alternate:
            out["rows"] += run_alternate(curve, [int(c) for c in a.counts.split(",")], a.reps)
            continue
        rows, (pp, vk, aff, w) = run(curve, [int(c) for c in a.counts.split(",")], a.reps)
        out["rows"] += rows
        if a.cpu_oracle:
            r = cpu_oracle(curve, pp, vk, aff, w)
            print(json.dumps(r), flush=True)
            out["rows"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
