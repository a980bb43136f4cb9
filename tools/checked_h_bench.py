"""The checked h chain against the unchecked one, the batched repair against single calls, and the checked prover against the
prover, on one GPU, same process, same buffers, alternating -- DESIGN.md 4.11.5.  A record; no threshold but one condition on
the batched repair (below).

usage: python tools/checked_h_bench.py [--quick] [--reps R] [--batch B] [--out FILE]      -> ONE JSON line
       python tools/checked_h_bench.py --parties [...]      the rows of the party-list forms, below

BN254, l = 2.  Rows (the yardstick of each is the unchanged call in the same run):
  circom_h     zk_circom_h against zk_circom_h_checked at log2_m = 15 (the SHA-256 proof's) and 20, all twelve masks: clean
               shares, and one lying party in round 1 (its rows of qap_a / qap_b / qap_c random: the unchecked call then computes
               garbage at the same cost, the checked one the honest h)
  repair       three zk_pss_repair calls against one zk_pss_repair_batch of three items on the same three matrices, clean, at
               2^14 and 2^19 chunks.  `yardstick_spread_us` is max - min of the three-single-calls windows of the same run;
               `batch_not_slower` is batch <= singles + that spread
  prove        zk_groth16_prove against zk_groth16_prove_checked on the SHA-256 instance, all masks, clean
A figure is the median over R windows of B back-to-back calls with one stream synchronise behind them (host clock / B; the
prover is synchronous: B = 1 call per window there); the entry points of a row take turns window by window
(tools/checked_king_bench.py's method).

--parties (party BAD absent; profiles/checked_h_parties_bench.json):
  repair       three zk_pss_repair_parties calls against one zk_pss_repair_batch_parties of three items on the same compact
               matrices, clean, at 2^14 and 2^19 chunks; the same `batch_not_slower` condition
  circom_h     at log2_m = 15 and 20: zk_circom_h; zk_circom_h_checked clean; zk_circom_h_checked with one liar in round 1;
               zk_circom_h_checked_parties with that liar left out (on the liar's input: its rows are not read) -- the four
               taking turns; ratios against zk_circom_h
  prove        zk_groth16_prove against zk_groth16_prove_checked_parties with one party absent, SHA-256 instance"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zksaas_amd as zk
from zksaas_amd import api
from zksaas_amd import groth16 as zg

L = 2
BAD = 3


def raw(rng, count):
    """random field elements as Montgomery limbs: anything below 2^252 is below every scalar modulus here"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def windows(pp, fns, reps, batch, spread=False):
    """median seconds per call of each fn, the fns taking turns window by window; spread: also max - min per fn"""
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
    med = [sorted(t)[len(t) // 2] for t in ts]
    return (med, [max(t) - min(t) for t in ts]) if spread else med


def us(t):
    return round(t * 1e6, 2)


def honest(pp, nch, rng, seed):
    return pp.pack(zk.DeviceBuffer.from_numpy(pp, raw(rng, nch * L)), nch, seed=seed).to_numpy().reshape(pp.n, nch, 4)


def summaries(pp, rep):
    w = 3 + pp.n
    flat = [int(v) for v in rep.summary_d.to_numpy(np.uint64)]
    return [flat[i:i + w] for i in range(0, len(flat), w)]


def circom_h_row(pp, log_m, reps, batch):
    n, nch = pp.n, (1 << log_m) // L
    rng = np.random.default_rng(log_m)
    rows = [honest(pp, nch, rng, 1 + k) for k in range(3)]
    masks = zg.ProofMasks(pp, log_m, 5)
    mk = C.byref(masks.ct)
    hu, hc = pp.alloc_fr(n * nch), pp.alloc_fr(n * nch)
    rep = api.h_report(pp, log_m)
    res = {"log2_m": log_m, "chunks": nch}
    want = None
    for leg in ("clean", "one_liar_round_1"):
        if leg != "clean":
            rows = [r.copy() for r in rows]
            for r in rows:
                r[BAD] = raw(rng, nch)
        q = [zk.DeviceBuffer.from_numpy(pp, r) for r in rows]

        def unchecked():
            pp._check(pp.lib.zk_circom_h(pp.h, q[0].ptr, q[1].ptr, q[2].ptr, log_m, mk, 7, hu.ptr, None))

        def checked():
            pp._check(pp.lib.zk_circom_h_checked(pp.h, q[0].ptr, q[1].ptr, q[2].ptr, log_m, mk, 7, hc.ptr, rep.status.ptr,
                                                 rep.errpos.ptr, rep.summary_d.ptr, None))

        tu, tc = windows(pp, [unchecked, checked], reps, batch)
        heads = [s[:3] for s in summaries(pp, rep)]
        if leg == "clean":      # (the shares' randomness is the production stream: outputs are compared as secrets)
            want = pp.unpack(hu, nch).to_numpy().copy()
            assert heads == [[nch, 0, 0]] * 7, heads
        else:
            assert heads == [[0, nch, 0]] * 3 + [[nch, 0, 0]] * 4, heads
        assert np.array_equal(pp.unpack(hc, nch).to_numpy(), want), leg               # the honest h
        res[leg] = {"unchecked_us": us(tu), "checked_us": us(tc), "ratio": round(tc / tu, 3), "overhead_us": us(tc - tu)}
    return res


def repair_row(pp, log_chunks, reps, batch):
    n, nch, k = pp.n, 1 << log_chunks, 2 * L
    rng = np.random.default_rng(100 + log_chunks)
    per = n * nch
    words = np.concatenate([honest(pp, nch, rng, 10 + i).reshape(per, 4) for i in range(3)])
    sh = zk.DeviceBuffer.from_numpy(pp, words)
    one = [(zk.DeviceBuffer(pp, nch), zk.DeviceBuffer(pp, 4 * nch), zk.DeviceBuffer(pp, 8 * (3 + n))) for _ in range(3)]
    st, ep, sm = zk.DeviceBuffer(pp, 3 * nch), zk.DeviceBuffer(pp, 12 * nch), zk.DeviceBuffer(pp, 24 * (3 + n))

    def singles():
        for i in range(3):
            pp._check(pp.lib.zk_pss_repair(pp.h, sh.ptr + i * per * 32, nch, k, one[i][0].ptr, one[i][1].ptr, one[i][2].ptr,
                                           None))

    def batched():
        pp._check(pp.lib.zk_pss_repair_batch(pp.h, sh.ptr, per, 3, nch, k, st.ptr, ep.ptr, sm.ptr, None))

    (ts, tb), (spread, _) = windows(pp, [singles, batched], reps, batch, spread=True)
    flat = [int(v) for v in sm.to_numpy(np.uint64)]
    assert [flat[i * (3 + n):i * (3 + n) + 3] for i in range(3)] == [[nch, 0, 0]] * 3
    assert all([int(v) for v in o[2].to_numpy(np.uint64)][:3] == [nch, 0, 0] for o in one)
    return {"log2_chunks": log_chunks, "three_singles_us": us(ts), "batch_of_three_us": us(tb), "ratio": round(tb / ts, 3),
            "saved_us": us(ts - tb), "yardstick_spread_us": us(spread), "batch_not_slower": bool(tb <= ts + spread)}


def parties_repair_row(pp, log_chunks, reps, batch):
    n, nch, k = pp.n, 1 << log_chunks, 2 * L
    rng = np.random.default_rng(200 + log_chunks)
    S = [p for p in range(n) if p != BAD]
    np_ = len(S)
    per = np_ * nch
    ids = (C.c_uint32 * np_)(*S)
    words = np.concatenate([honest(pp, nch, rng, 20 + i)[S].reshape(per, 4) for i in range(3)])
    sh = zk.DeviceBuffer.from_numpy(pp, words)
    one = [(zk.DeviceBuffer(pp, nch), zk.DeviceBuffer(pp, 4 * nch), zk.DeviceBuffer(pp, 8 * (3 + n))) for _ in range(3)]
    st, ep, sm = zk.DeviceBuffer(pp, 3 * nch), zk.DeviceBuffer(pp, 12 * nch), zk.DeviceBuffer(pp, 24 * (3 + n))

    def singles():
        for i in range(3):
            pp._check(pp.lib.zk_pss_repair_parties(pp.h, sh.ptr + i * per * 32, ids, np_, nch, k, one[i][0].ptr, one[i][1].ptr,
                                                   one[i][2].ptr, None))

    def batched():
        pp._check(pp.lib.zk_pss_repair_batch_parties(pp.h, sh.ptr, ids, np_, per, 3, nch, k, st.ptr, ep.ptr, sm.ptr, None))

    (ts, tb), (spread, _) = windows(pp, [singles, batched], reps, batch, spread=True)
    flat = [int(v) for v in sm.to_numpy(np.uint64)]
    assert [flat[i * (3 + n):i * (3 + n) + 3] for i in range(3)] == [[nch, 0, 0]] * 3
    assert all([int(v) for v in o[2].to_numpy(np.uint64)][:3] == [nch, 0, 0] for o in one)
    return {"log2_chunks": log_chunks, "absent": BAD, "three_singles_us": us(ts), "batch_of_three_us": us(tb),
            "ratio": round(tb / ts, 3), "saved_us": us(ts - tb), "yardstick_spread_us": us(spread),
            "batch_not_slower": bool(tb <= ts + spread)}


def parties_circom_h_row(pp, log_m, reps, batch):
    n, nch = pp.n, (1 << log_m) // L
    rng = np.random.default_rng(300 + log_m)
    rows = [honest(pp, nch, rng, 1 + k) for k in range(3)]
    masks = zg.ProofMasks(pp, log_m, 5)
    mk = C.byref(masks.ct)
    hu, hc, hl, hp = (pp.alloc_fr(n * nch) for _ in range(4))
    rc, rl, rp = (api.h_report(pp, log_m) for _ in range(3))
    S = [p for p in range(n) if p != BAD]
    ids = (C.c_uint32 * len(S))(*S)
    q = [zk.DeviceBuffer.from_numpy(pp, r) for r in rows]
    bad = [r.copy() for r in rows]
    for r in bad:
        r[BAD] = raw(rng, nch)
    qb = [zk.DeviceBuffer.from_numpy(pp, r) for r in bad]

    def unchecked():
        pp._check(pp.lib.zk_circom_h(pp.h, q[0].ptr, q[1].ptr, q[2].ptr, log_m, mk, 7, hu.ptr, None))

    def checked(src, h, rep):
        return lambda: pp._check(pp.lib.zk_circom_h_checked(pp.h, src[0].ptr, src[1].ptr, src[2].ptr, log_m, mk, 7, h.ptr,
                                                            rep.status.ptr, rep.errpos.ptr, rep.summary_d.ptr, None))

    def listed():
        pp._check(pp.lib.zk_circom_h_checked_parties(pp.h, ids, len(S), qb[0].ptr, qb[1].ptr, qb[2].ptr, log_m, mk, 7, hp.ptr,
                                                     rp.status.ptr, rp.errpos.ptr, rp.summary_d.ptr, None))

    tu, tc, tl, tp = windows(pp, [unchecked, checked(q, hc, rc), checked(qb, hl, rl), listed], reps, batch)
    want = pp.unpack(hu, nch).to_numpy().copy()
    for h in (hc, hl, hp):
        assert np.array_equal(pp.unpack(h, nch).to_numpy(), want)                       # the honest h
    assert [x[:3] for x in summaries(pp, rc)] == [[nch, 0, 0]] * 7
    assert [x[:3] for x in summaries(pp, rl)] == [[0, nch, 0]] * 3 + [[nch, 0, 0]] * 4
    assert [x[:3] for x in summaries(pp, rp)] == [[nch, 0, 0]] * 6 + [[0, 0, 0]]       # no chunk reaches stage 2
    return {"log2_m": log_m, "chunks": nch, "absent": BAD, "unchecked_us": us(tu), "checked_clean_us": us(tc),
            "checked_one_liar_us": us(tl), "checked_parties_liar_out_us": us(tp), "ratio_clean": round(tc / tu, 3),
            "ratio_one_liar": round(tl / tu, 3), "ratio_parties": round(tp / tu, 3),
            "parties_over_clean": round(tp / tc, 3), "parties_over_one_liar": round(tp / tl, 3)}


def parties_prove_row(pp, reps):
    from zksaas_amd import sha256_circuit as sc
    from zksaas_amd.fields import FR
    p = FR["bn254"]
    r1, w = sc.build(1, 2, p, pad_wires=sc.REFERENCE_WIRES)
    rng = np.random.default_rng(42)
    td = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(5)]
    crs = zg.Crs(pp, zg.SetupScalars("bn254", r1, *td))
    wit = zg.Witness(pp, "bn254", r1, w, seed=43)
    r, s = (int.from_bytes(rng.bytes(32), "little") % p for _ in range(2))
    masks = zg.ProofMasks(pp, wit.log_m, seed=77)
    S = [q for q in range(pp.n) if q != BAD]
    last = {}

    def unchecked():
        last["u"] = zg.prove(pp, crs, wit, r, s, masks=masks, seed=9)

    def listed():
        last["p"] = zg.prove(pp, crs, wit, r, s, masks=masks, seed=9, check=True, parties=S)

    tu, tp = windows(pp, [unchecked, listed], reps, 1)
    nch = (1 << wit.log_m) // L
    assert [x[:3] for x in summaries(pp, last["p"][1])] == [[nch, 0, 0]] * 6 + [[0, 0, 0]]
    return {"log2_m": wit.log_m, "absent": BAD, "unchecked_ms": round(tu * 1e3, 3), "checked_parties_ms": round(tp * 1e3, 3),
            "ratio": round(tp / tu, 3), "overhead_us": us(tp - tu)}


def prove_row(pp, reps):
    from zksaas_amd import sha256_circuit as sc
    from zksaas_amd.fields import FR
    p = FR["bn254"]
    r1, w = sc.build(1, 2, p, pad_wires=sc.REFERENCE_WIRES)
    rng = np.random.default_rng(42)
    td = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(5)]
    crs = zg.Crs(pp, zg.SetupScalars("bn254", r1, *td))
    wit = zg.Witness(pp, "bn254", r1, w, seed=43)
    r, s = (int.from_bytes(rng.bytes(32), "little") % p for _ in range(2))
    masks = zg.ProofMasks(pp, wit.log_m, seed=77)
    last = {}

    def unchecked():
        last["u"] = zg.prove(pp, crs, wit, r, s, masks=masks, seed=9)

    def checked():
        last["c"] = zg.prove(pp, crs, wit, r, s, masks=masks, seed=9, check=True)

    tu, tc = windows(pp, [unchecked, checked], reps, 1)
    rep = last["c"][1]
    nch = (1 << wit.log_m) // L
    assert [x[:3] for x in summaries(pp, rep)] == [[nch, 0, 0]] * 7
    return {"log2_m": wit.log_m, "unchecked_ms": round(tu * 1e3, 3), "checked_ms": round(tc * 1e3, 3),
            "ratio": round(tc / tu, 3), "overhead_us": us(tc - tu)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--no-prove", action="store_true")
    ap.add_argument("--parties", action="store_true", help="the rows of the party-list forms (DESIGN.md 4.11.6)")
    ap.add_argument("--out")
    a = ap.parse_args()
    pp = zk.PackedSharingParams("bn254", L)
    out = {"tool": "checked_h_bench", "curve": "bn254", "l": L, "reps": a.reps, "batch": a.batch}
    if a.parties:
        out["mode"] = "parties"
        out["repair"] = [parties_repair_row(pp, lg, a.reps, a.batch) for lg in ([14] if a.quick else [14, 19])]
        out["circom_h"] = [parties_circom_h_row(pp, lg, a.reps, a.batch) for lg in ([15] if a.quick else [15, 20])]
        if not a.no_prove:
            out["prove"] = parties_prove_row(pp, a.reps)
        return emit(out, a.out)
    out["repair"] = [repair_row(pp, lg, a.reps, a.batch) for lg in ([14] if a.quick else [14, 19])]
    out["circom_h"] = [circom_h_row(pp, lg, a.reps, a.batch) for lg in ([15] if a.quick else [15, 20])]
    if not a.no_prove:
        out["prove"] = prove_row(pp, a.reps)
    emit(out, a.out)


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
