"""The dealer's kernels, timed on one GPU: what the reference does ONCE per circuit / per proof
before the parties start, and calls its slowest step (`groth16/src/proving_key.rs:47-123`, `.github/workflows/ci.yml:54-67`).

usage: python tools/dealer_bench.py [--quick] [--reps R]      -> ONE JSON line (`bench.py --workload dealer` prints the same)
       python tools/dealer_bench.py setup_scalars [--reps R]  -> ONE JSON line with the `setup_scalars` entry alone

Keys (per entry: wall per call with a sync on both sides, units / s, the base-field products one unit costs as the
kernel executes them, and `frac_issue_bound` = products / s over the multiplier's issue bound -- 153.6 G/s for 8 limbs,
68.3 G/s for 12 limbs; these kernels are multiplier-bound, HBM traffic is a few hundred bytes per ~10^3 products):
  crs_pack_points   `pack_from_arkworks_proving_key` at the SHA-256 circuit's sizes: det_pack over group elements of
                    a_query[1..], b_g1_query[1..], l_query, h_query (G1) and b_g2_query[1..] (G2), chunks of l = 2 -> n = 8
  fixed_base_mul    scalars -> multiples of a generator (the trapdoor dealer; `proving_key.rs:125-176` `rand()` dummy CRS)
  msm_table_build   zk_msm_precompute over the five packed query vectors
  fft_mask_sample   `FftMask::sample` (`dfft/mod.rs:30-85`) at 2^15 and 2^20
  degred_mask_sample / msm_mask_sample   `deg_red.rs:40-66`, `dmsm/mod.rs:21-47`
  proof_masks       the twelve masks of a proof at the SHA-256 proof's size (log_m = 15, sha256.rs:226-291): ms per mask set
                    through the twelve single sampler calls (`twelve_calls`), through zk_groth16_deal_masks at nproofs = 1 and
                    8 (`deal_b1`, `deal_b8`: median, min and max of the repetitions, per set), mask sets per second, and the
                    MsmMask part alone on the host (five zk_msm_mask_sample) against the device (deal_masks with only the MSM
                    slots set) -- all in this process, every path writing into buffers allocated before the clock starts
  witness_deal      ms per witness of the SHA-256 circuit: the former composition (zk_r1cs_qap, zk_bitrev, zk_pss_pack, the
                    witness downloaded, sliced and padded in Python and uploaded again) against zk_groth16_deal_witness
  setup_scalars     (its own mode) the circuit-specific setup of the SHA-256 circuit in the exponent: groth16.SetupScalars on
                    the host plus the upload of its five vectors (one run: it takes seconds) against groth16.DeviceSetup
                    (zk_groth16_setup_scalars, wall clock around a stream sync), the upload of the C matrix it needs, and the
                    longest column of A, B and C (a host count: what the long-column path of the kernels is there for)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zksaas_amd as zk
from zksaas_amd import api, synthetic
from zksaas_amd import groth16 as zg

ISSUE_BOUND = {8: 153.6e9, 12: 153.6e9 * (2 * 64 + 8) / (2 * 144 + 12)}     # products / s: 2 N^2 + N multiply instructions each
# base-field products per group operation as executed (api.MULS_PER_ADD; doubling dbl-2008-s-1: 8.5 / 3 x for Fq2)
MADD = {api.ZK_G1: 9.47, api.ZK_G2: 23.76}
DBL = {api.ZK_G1: 8.5, api.ZK_G2: 21.0}


def timed(pp, fn, reps):
    fn()
    pp.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        pp.sync()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def timed_spread(pp, fn, reps):
    """median, min, max of `reps` synchronised calls (after one warm-up call)"""
    fn()
    pp.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        pp.sync()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def ms3(t, per=1):
    return {"ms": round(t[0] / per * 1e3, 4), "min_ms": round(t[1] / per * 1e3, 4), "max_ms": round(t[2] / per * 1e3, 4)}


def twelve_call_masks(pp, log_m, seed, g1, g2, pm, w2m):
    """The composition zk_groth16_deal_masks replaces: six zk_fft_mask_sample, one zk_degred_mask_sample, five
    zk_msm_mask_sample (ProofMasks before the batched dealer), written into the preallocated buffers of `pm` -- no
    allocation, no root-of-unity power and no generator encoding inside, as for the batched call it is compared with.
    w2m: the encoded 2m-th root of unity."""
    lib, h = pp.lib, pp.h
    for k in range(6):
        pp._check(lib.zk_fft_mask_sample(h, int(k < 3), w2m.ctypes.data if k < 3 else None, int(k < 3), log_m, seed + k,
                                         pm.fft[k].in_mask.ptr, pm.fft[k].out_mask.ptr, None))
    pp._check(lib.zk_degred_mask_sample(h, (1 << log_m) // pp.l, seed + 6, pm.degred.in_mask.ptr, pm.degred.out_mask.ptr, None))
    twelve_call_msm(pp, seed, g1, g2, pm)


def twelve_call_msm(pp, seed, g1, g2, pm):
    for k in range(5):
        pp._check(pp.lib.zk_msm_mask_sample(pp.h, api.ZK_G2 if k == 2 else api.ZK_G1, (g2 if k == 2 else g1).ctypes.data, seed + 7 + k,
                                            pm.msm[k].in_mask.ctypes.data, pm.msm[k].out_mask.ctypes.data))


def proof_masks_entry(pp, reps):
    import ctypes as C
    log_m = 15
    g1, g2 = (np.ascontiguousarray(g, dtype=np.uint64).reshape(-1) for g in zg.generators(pp))
    w2m = pp.fr.encode_one(zg._root_of_unity(pp.curve, log_m + 1))
    out = {"log_m": log_m}
    old_pm = zg.ProofMasks.__new__(zg.ProofMasks)
    old_pm._alloc(pp, log_m)
    out["twelve_calls"] = ms3(timed_spread(pp, lambda: twelve_call_masks(pp, log_m, 77, g1, g2, old_pm, w2m), reps))
    for nb in (1, 8):
        sets, arr = [], (zg.Masks * nb)()
        for b in range(nb):
            pm = zg.ProofMasks.__new__(zg.ProofMasks)
            pm._alloc(pp, log_m)
            C.memmove(C.byref(arr, b * C.sizeof(zg.Masks)), C.byref(pm.ct), C.sizeof(zg.Masks))
            sets.append(pm)
        t = timed_spread(pp, lambda: api.deal_masks(pp, nb, log_m, g1, g2, 77, arr), reps)
        e = ms3(t, nb)
        e["mask_sets_per_s"] = round(nb / t[0], 1)
        out["deal_b%d" % nb] = e
        if nb == 8:                                   # the MsmMask part alone: only the MSM slots set
            for b in range(nb):
                for k in range(6):
                    arr[b].fft_in[k] = arr[b].fft_out[k] = None
                arr[b].degred_in = arr[b].degred_out = None
            t = timed_spread(pp, lambda: api.deal_masks(pp, nb, log_m, g1, g2, 77, arr), reps)
            out["msm_mask_device_b8"] = ms3(t, nb)
        else:
            one = zg.Masks()
            C.memmove(C.byref(one), C.byref(arr[0]), C.sizeof(one))
            for k in range(6):
                one.fft_in[k] = one.fft_out[k] = None
            one.degred_in = one.degred_out = None
            out["msm_mask_device_b1"] = ms3(timed_spread(pp, lambda: api.deal_masks(pp, 1, log_m, g1, g2, 77, one), reps))
        del sets
    out["msm_mask_host"] = ms3(timed_spread(pp, lambda: twelve_call_msm(pp, 77, g1, g2, old_pm), reps))
    out["speedup_b1"] = round(out["twelve_calls"]["ms"] / out["deal_b1"]["ms"], 2)
    out["speedup_b8"] = round(out["twelve_calls"]["ms"] / out["deal_b8"]["ms"], 2)
    # the pass condition: one call beats the twelve by more than the spread of the repetitions (slowest repetition of the
    # one against the fastest of the twelve), and a set of a batch of 8 costs no more than a set dealt alone
    out["b1_faster_beyond_spread"] = out["deal_b1"]["max_ms"] < out["twelve_calls"]["min_ms"]
    out["b8_no_dearer_than_b1"] = out["deal_b8"]["ms"] <= out["deal_b1"]["ms"]
    return out


def witness_deal_entry(pp, reps):
    from zksaas_amd import circom
    from zksaas_amd import sha256_circuit as sc
    r1, w = sc.build(1, 2, pp.fr.p)
    dev = circom.DeviceR1cs(pp, r1)
    w_d = pp.upload_fr(w)
    ni = r1.num_instance_variables

    def old():
        m = 1 << dev.log_m
        for k, d in enumerate(dev.qap(w_d)):
            pp._check(pp.lib.zk_bitrev(pp.h, d.ptr, dev.log_m, None))
            pp.pack(d, m // pp.l, 5 + k, order=1)
        wl = pp.download_fr(w_d, r1.num_variables)
        for vals, sd in ((wl[1:], 8), (wl[ni:], 9)):
            vals = list(vals)
            vals += [0] * (-len(vals) % pp.l)
            pp.pack(pp.upload_fr(vals), len(vals) // pp.l, sd)
    return {"circuit": "sha256", "log_m": dev.log_m, "num_variables": r1.num_variables,
            "r1cs_qap_bitrev_pack_python_padding": ms3(timed_spread(pp, old, max(2, reps // 2))),
            "deal_witness": ms3(timed_spread(pp, lambda: zg.Witness(pp, pp.curve, r1, w_d, 5, dev_r1cs=dev), reps))}


def setup_scalars_entry(pp, reps):
    from zksaas_amd import circom
    from zksaas_amd import sha256_circuit as sc
    p = pp.fr.p
    r1, _ = sc.build(1, 2, p)
    td = [pow(7, 11 + i, p) for i in range(5)]
    t0 = time.perf_counter()
    host = zg.SetupScalars(pp.curve, r1, *td)
    t1 = time.perf_counter()
    keep = [pp.upload_fr(v) for v in (host.a_query, host.b_query, host.l_query, host.h_query, host.gamma_abc)]
    pp.sync()
    t2 = time.perf_counter()
    del keep
    dev = circom.DeviceR1cs(pp, r1)
    t3 = time.perf_counter()
    dev.upload_c(r1)
    pp.sync()
    t4 = time.perf_counter()
    got = zg.DeviceSetup(pp, dev, *td).to_host()
    same = all(getattr(got, k) == getattr(host, k) for k in ("a_query", "b_query", "l_query", "h_query", "gamma_abc"))
    longest = {}
    for name, rows in (("a", r1.a), ("b", r1.b), ("c", r1.c)):
        cnt = {}
        for row in rows:
            for _, wire in row:
                cnt[wire] = cnt.get(wire, 0) + 1
        top = sorted(cnt.values(), reverse=True)
        longest[name] = {"nonzeros": sum(top), "longest_columns": top[:4],
                         "columns_above_heavy_min": sum(1 for v in top if v > zg.SETUP_HEAVY_MIN)}
    return {"circuit": "sha256", "log_m": dev.log_m, "num_variables": r1.num_variables, "num_constraints": r1.num_constraints,
            "host_setup_scalars_s": round(t1 - t0, 3), "host_upload_fr_s": round(t2 - t1, 3),
            "upload_c_matrix_s": round(t4 - t3, 3), "device_setup": ms3(timed_spread(pp, lambda: zg.DeviceSetup(pp, dev, *td), reps)),
            "device_equals_host": same, "heavy_min": zg.SETUP_HEAVY_MIN, "columns": longest}


def entry(dt, units, unit_name, products_per_unit, limbs, **extra):
    e = {"ms": round(dt * 1e3, 4), unit_name + "_per_s": round(units / dt, 1),
         "products_per_" + unit_name: round(products_per_unit, 1),
         "frac_issue_bound": round(units * products_per_unit / dt / ISSUE_BOUND[limbs], 4)}
    e.update(extra)
    return e


def random_points(pp, group, count, seed):
    return zg.base_points(pp, group, synthetic.rand_fr_device(pp, count, seed), count)


def pack_points_cost(group, nv, inv):
    """products per OUTPUT share of the form the kernel runs (see csrc/groth16.hpp); inv = products of one inversion"""
    ext = 3 if group == api.ZK_G2 else 1
    if nv == 2:      # joint sparse form: 257 doublings, ~128 mixed additions, the two-sum table (one inversion), normalisation
        return 257 * DBL[group] + 128.5 * MADD[group] + (2 * inv + 10) * ext
    return 256 * DBL[group] + 128 * nv * MADD[group] + inv * ext


def run(curve, quick, reps):
    pp = zk.PackedSharingParams(curve, 2)
    for kv in filter(None, os.environ.get("ZK_BENCH_OPTIONS", "").split(",")):     # A/B runs: name=value context options
        pp.set_option(kv.split("=")[0], int(kv.split("=")[1]))
    limbs = pp.fq.nl * 2                    # 32-bit limbs of the base field
    out = {"curve": curve, "base_field_limbs": limbs}
    # what the kernels run (csrc/groth16.hpp, csrc/ec.hpp, round 6): divstep inversion (~35 / 25 product equivalents of issue on
    # 8 / 12 limbs), 16-bit windows from 2^19 scalars up, joint-sparse-form packing
    info = {"inversion": "safegcd", "base_mul_wide_from": 1 << 19, "pack_points_form": "jsf"}
    out["build"] = info
    inv = 35.0 if limbs == 8 else 25.0
    # ---- CRS share packing at the SHA-256 circuit's sizes (proving_key.rs:47-123)
    sizes = [("a_query", api.ZK_G1, 14911), ("b_g1_query", api.ZK_G1, 14911), ("l_query", api.ZK_G1, 14910),
             ("h_query", api.ZK_G1, 16384), ("b_g2_query", api.ZK_G2, 14911)]
    if curve != "bn254" or quick:
        sizes = [("h_query", api.ZK_G1, 16384), ("b_g2_query", api.ZK_G2, 14911)]
    crs, total = {}, 0.0
    for name, grp, nch in sizes:
        pts = random_points(pp, grp, nch * pp.l, 100 + nch)
        dt = timed(pp, lambda: zg.pack_points(pp, grp, pts, nch, pp.l).free(), reps)
        crs[name] = entry(dt, nch * pp.n, "share", pack_points_cost(grp, pp.l, inv), limbs, chunks=nch,
                          group="G2" if grp == api.ZK_G2 else "G1")
        total += dt
        pts.free()
    out["crs_pack_points"] = {"vectors": crs, "total_ms": round(total * 1e3, 3)}

    # ---- fixed-base multiplication
    fb = {}
    big = 20 if quick else (22 if curve == "bn254" else 24)
    for grp, gname in ((api.ZK_G1, "G1"), (api.ZK_G2, "G2")):
        for log_n in (17, big):
            cnt = 1 << log_n
            sc = synthetic.rand_fr_device(pp, cnt, 7 + log_n)
            dt = timed(pp, lambda: zg.base_points(pp, grp, sc, cnt).free(), max(2, reps // 2))
            nwin = 32
            if info.get("base_mul_wide_from") and cnt >= info["base_mul_wide_from"]:
                nwin = 16
            fb["%s_2^%d" % (gname, log_n)] = entry(dt, cnt, "point", nwin * MADD[grp] + inv * (3 if grp == api.ZK_G2 else 1),
                                                   limbs, windows=nwin)
            sc.free()
    out["fixed_base_mul"] = fb

    # ---- fixed-base MSM tables over packed query vectors (zk_msm_precompute)
    tb = {}
    for grp, gname, nch in ((api.ZK_G1, "G1", 16384), (api.ZK_G2, "G2", 14911)):
        pts = random_points(pp, grp, nch * pp.n, 300 + nch)

        def build():
            api.msm_precompute(pp, grp, pts, nch * pp.n)
            api.msm_forget(pp, pts)
        dt = timed(pp, build, max(2, reps // 2))
        api.msm_precompute(pp, grp, pts, nch * pp.n)
        ti = api.msm_table_info(pp, grp, pts)
        api.msm_forget(pp, pts)
        tb[gname] = entry(dt, nch * pp.n, "point", 254 * DBL[grp] + ti["windows"] * inv * (3 if grp == api.ZK_G2 else 1), limbs, **ti)
        pts.free()
    out["msm_table_build"] = tb

    # ---- masks
    fm = {}
    for log_m in ((15,) if quick else (15, 20)):
        for rearr, inverse in ((True, True), (False, False)):
            g = 5 if inverse else None

            def sample():
                m_ = zk.FftMask.sample(pp, rearr, g, inverse, log_m, 9)
                m_.in_mask.free(), m_.out_mask.free()
            dt = timed(pp, sample, reps)
            m = 1 << log_m
            fm["2^%d_%s" % (log_m, "ifft_rearranged" if inverse else "fft")] = {
                "ms": round(dt * 1e3, 4), "elements_per_s": round(m / dt, 1),
                "algorithmic_bytes": 2 * pp.n * (m // pp.l) * 32, "frac_hbm": round(2 * pp.n * (m // pp.l) * 32 / dt / 8e12, 4)}
    out["fft_mask_sample"] = fm

    def dm():
        k = zk.DegRedMask.sample(pp, 1 << 14, 10)
        k.in_mask.free(), k.out_mask.free()
    dt = timed(pp, dm, reps)
    out["degred_mask_sample_2^14"] = {"ms": round(dt * 1e3, 4), "chunks_per_s": round((1 << 14) / dt, 1)}
    gen = zg._affine_codec(pp, list(zg.G1_GEN[pp.curve]), False)
    dt = timed(pp, lambda: zk.MsmMask.sample(pp, api.ZK_G1, gen, 11), reps)
    out["msm_mask_sample_g1"] = {"ms": round(dt * 1e3, 4)}
    out["proof_masks"] = proof_masks_entry(pp, max(reps, 9))
    if curve == "bn254":                              # (the SHA-256 circuit is built over BN254's scalar field)
        out["witness_deal"] = witness_deal_entry(pp, reps)
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    quick = "--quick" in argv
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    if "setup_scalars" in argv:
        res = {"workload": "dealer: circuit-specific setup in the exponent (SHA-256 circuit, BN254)",
               "setup_scalars": setup_scalars_entry(zk.PackedSharingParams("bn254", 2), reps)}
        print(json.dumps(res), flush=True)
        return res
    res = {"workload": "dealer (SURVEY.md 8 f1 / f2): CRS share packing, fixed-base multiplication, table build, mask sampling",
           "curves": [run("bn254", quick, reps), run("bls12_381", quick, reps)]}
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
