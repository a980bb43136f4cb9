"""Worker of tests/test_gpu_party.py: one rank of the star network whose k parties are driven by k host threads through the
per-party entry points (zk_party_*, zksaas_amd.net.Party); BN254, l = 2, n = 8, replayable randomness.  Every rank deals the
SAME seeded inputs.  A scenario sends the parent (rank, verdict, details, data): `data` holds result rows by party id, so
that the parent can compare scenarios with each other (two ranks of four threads against one rank of eight).
Every thread is joined with a deadline: a deadlock is a failed check within seconds, nothing is tried again."""
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 5                      # the coset shift of the d_ifft cases
JOIN_S = 60.0              # what the threads of one step may take together


def run_threads(fns, limit=JOIN_S):
    """run the callables on a thread each; -> their results.  A thread that is not back at the deadline fails the step."""
    res, errs = [None] * len(fns), [None] * len(fns)

    def wrap(i):
        try:
            res[i] = fns[i]()
        except BaseException as e:      # noqa: BLE001
            errs[i] = e

    ths = [threading.Thread(target=wrap, args=(i,), daemon=True) for i in range(len(fns))]
    for t in ths:
        t.start()
    deadline = time.monotonic() + limit
    for t in ths:
        t.join(max(0.0, deadline - time.monotonic()))
    stuck = [i for i, t in enumerate(ths) if t.is_alive()]
    assert not stuck, "threads %r did not return within %.0f s (deadlock?)" % (stuck, limit)
    return res, errs


def run(rank, world, net_ids, scenario, q, transport="shm", barrier=None):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        import zksaas_amd as zk
        from zksaas_amd import groth16 as zg
        from zksaas_amd import net as znet
        from zksaas_amd.api import ZK_G1, ZK_G2, DegRedMask, DeviceBuffer, FftMask, MsmMask
        from oracle.curve import g1, g2
        from oracle.params import BN254
        from oracle.prng import rand_fp
        from gpu_util import dec_jacobian
        from test_oracle_groth16 import small_r1cs

        zk.api.DEFAULT_OPTIONS["rng_replay"] = 1     # a spawned process: the parent's conftest does not reach here
        pp = zk.PackedSharingParams("bn254", 2)
        mode = "block" if scenario.startswith("block") else "staged"
        timeout_ms = 2000 if scenario == "away" else 5000
        net = znet.StarNet(pp, rank, world, net_ids[0], transport, timeout_ms=timeout_ms)
        k, n, l = net.k, pp.n, pp.l
        sel = list(net.parties)
        eb = pp.fr.nbytes
        G1, G2 = g1(BN254), g2(BN254)
        checks, data = {}, {}

        def raw(seed, count):
            a = np.random.default_rng(seed).integers(0, 1 << 62, size=(count, 4), dtype=np.uint64)
            a[:, 3] &= np.uint64((1 << 60) - 1)
            return a

        def bytes_of(x, row_bytes):
            """[n][row_bytes] uint8 of a full party-major vector (numpy limbs or a device buffer)"""
            if isinstance(x, DeviceBuffer):
                x = x.to_numpy(np.uint8)
            return np.ascontiguousarray(x).view(np.uint8).reshape(n, row_bytes)

        def block_of(x, row_bytes):
            """this rank's rows of a full vector as ONE device block [k][row]: what the rank call takes"""
            return DeviceBuffer.from_numpy(pp, np.ascontiguousarray(bytes_of(x, row_bytes)[sel]))

        def rows_of(x, row_bytes, how=None):
            """this rank's rows as k device buffers: carved from one block, or allocated one by one (with a gap behind each,
            so that two allocations can never happen to be the rows of one block)"""
            if x is None:
                return [None] * k
            if (how or mode) == "block":
                b = block_of(x, row_bytes)
                return [b.view(i * row_bytes, row_bytes) for i in range(k)]
            full = bytes_of(x, row_bytes)
            out = []
            for p_ in sel:
                b = DeviceBuffer(pp, row_bytes + 256)
                pp._check(pp.lib.zk_memcpy_h2d(pp.h, b.ptr, np.ascontiguousarray(full[p_]).ctypes.data, row_bytes, None))
                out.append(b.view(0, row_bytes))
            return out

        def empty_rows(row_bytes):
            return rows_of(np.zeros((n, row_bytes), np.uint8), row_bytes)

        def host(rows, row_bytes):
            return np.stack([r.to_numpy(np.uint8)[:row_bytes] for r in rows])

        def mask_rows(m, row_bytes, cls):
            if m is None:
                return [None] * k
            a, b = rows_of(m.in_mask, row_bytes), rows_of(m.out_mask, row_bytes)
            return [cls(a[i], b[i]) for i in range(k)]

        def mask_block(m, row_bytes, cls):
            return None if m is None else cls(block_of(m.in_mask, row_bytes), block_of(m.out_mask, row_bytes))

        parties = [net.party(p_) for p_ in sel]
        stats0 = net.party_stats()

        def per_party(fn, limit=JOIN_S):
            """fn(i, party) on a thread per party; raises the first error"""
            res, errs = run_threads([lambda i=i: fn(i, parties[i]) for i in range(k)], limit)
            for e in errs:
                if e is not None:
                    raise e
            return res

        def same_point(a, b, is2):
            return (G2 if is2 else G1).eq(dec_jacobian(pp, a, is2), dec_jacobian(pp, b, is2))

        # ------------------------------------------------------------------ the transforms
        def fft_case(log_m, inverse, sid=0, seed=3, how=None, keep=None):
            Lc = (1 << log_m) // l
            x = raw(1000 + 10 * log_m + int(inverse) + 100 * sid, n * Lc)
            mk = None
            if log_m >= 6:
                mk = FftMask.sample(pp, bool(inverse), G if inverse else None, int(inverse), log_m, 40 + log_m)
            ref = block_of(x, Lc * eb)
            mb = mask_block(mk, Lc * eb, FftMask) or FftMask.zero()
            if inverse:
                znet.dist_d_ifft(pp, net, sid, ref, mb, True, log_m, g=G, seed=seed)
            else:
                znet.dist_d_fft(pp, net, sid, ref, mb, False, log_m, seed=seed)
            rows = rows_of(x, Lc * eb, how)
            mr = mask_rows(mk, Lc * eb, FftMask)

            def one(i, pt):
                m_ = mr[i] or FftMask.zero()
                if inverse:
                    pt.d_ifft(sid, rows[i], m_, True, log_m, g=G, seed=seed)
                else:
                    pt.d_fft(sid, rows[i], m_, False, log_m, seed=seed)
            per_party(one)
            pp.sync()
            got = host(rows, Lc * eb)
            if keep:
                data[keep] = {sel[i]: got[i] for i in range(k)}
            return np.array_equal(got, ref.to_numpy(np.uint8).reshape(k, Lc * eb))

        def prover_case(keep=None):
            r1, wv = small_r1cs()
            P = BN254.r
            td = [rand_fp(42, i, P) for i in range(5)]
            setup = zg.SetupScalars("bn254", r1, *td)
            crs = zg.Crs(pp, setup)
            wit = zg.Witness(pp, "bn254", r1, wv, seed=5)
            masks = zg.ProofMasks(pp, setup.log_m, seed=500)
            r, s = rand_fp(43, 0, P), rand_fp(43, 1, P)
            Lc = (1 << wit.log_m) // l
            e1, e2 = 2 * pp.fq.nbytes, 4 * pp.fq.nbytes
            cr = [rows_of(v, ln * w) for v, ln, w in ((crs.s, crs.len_a, e1), (crs.h, crs.len_a, e1), (crs.v, crs.len_a, e2),
                                                      (crs.w, crs.len_w, e1), (crs.u, crs.len_u, e1))]
            qap = [rows_of(v, Lc * eb) for v in wit.qap]
            a_sh, ax_sh = rows_of(wit.a_share, wit.len_a * eb), rows_of(wit.ax_share, wit.len_w * eb)
            fin = [rows_of(masks.fft[j].in_mask, Lc * eb) for j in range(6)]
            fout = [rows_of(masks.fft[j].out_mask, Lc * eb) for j in range(6)]
            din, dout = rows_of(masks.degred.in_mask, Lc * eb), rows_of(masks.degred.out_mask, Lc * eb)
            s1, s2 = crs.s1, crs.s2
            keepalive = []

            def one(i, pt):
                ct = zg.CrsShare(cr[0][i].ptr, cr[1][i].ptr, cr[2][i].ptr, cr[3][i].ptr, cr[4][i].ptr, crs.len_a, crs.len_w, crs.len_u,
                                 s1[0].ctypes.data, s1[1].ctypes.data, s1[2].ctypes.data, s1[3].ctypes.data, s1[4].ctypes.data,
                                 s2[0].ctypes.data, s2[1].ctypes.data, s2[2].ctypes.data)
                mk = zg.Masks()
                for j in range(6):
                    mk.fft_in[j], mk.fft_out[j] = fin[j][i].ptr, fout[j][i].ptr
                mk.degred_in, mk.degred_out = din[i].ptr, dout[i].ptr
                hm = []
                for j in range(5):
                    a = np.ascontiguousarray(masks.msm[j].in_mask[sel[i]])
                    b = np.ascontiguousarray(masks.msm[j].out_mask[sel[i]])
                    hm += [a, b]
                    mk.msm_in[j], mk.msm_out[j] = a.ctypes.data, b.ctypes.data
                keepalive.append((ct, mk, hm))
                return pt.prove(ct, [qap[0][i], qap[1][i], qap[2][i]], a_sh[i], ax_sh[i], r, s, wit.log_m, masks=mk, seed=9)
            got = per_party(one)
            if keep:
                data[keep] = {sel[i]: got[i] for i in range(k)}
            return crs, setup, wit, masks, r, s, wv, got

        if scenario in ("staged", "block"):
            # ---- every call, eight threads; each party's output is its row of the rank call on the same inputs and seed
            for log_m in (1, 6, 10):
                checks["d_fft_%d" % log_m] = fft_case(log_m, False, keep="d_fft_10" if log_m == 10 else None)
                checks["d_ifft_%d" % log_m] = fft_case(log_m, True, sid=1)
            for ln in (1, 33, 1000):
                x = raw(2000 + ln, n * ln)
                dm = DegRedMask.sample(pp, ln, 50 + ln)
                ref = znet.dist_deg_red(pp, net, 2, block_of(x, ln * eb), mask_block(dm, ln * eb, DegRedMask), ln, seed=8)
                rows, mr = rows_of(x, ln * eb), mask_rows(dm, ln * eb, DegRedMask)
                per_party(lambda i, pt: pt.deg_red(2, rows[i], mr[i], ln, seed=8))
                pp.sync()
                checks["deg_red_%d" % ln] = np.array_equal(host(rows, ln * eb), ref.to_numpy(np.uint8).reshape(k, ln * eb))
            ln = 33
            ns = pp.pack(DeviceBuffer.from_numpy(pp, raw(2100, l * ln)), ln, 60)
            ds = pp.pack(DeviceBuffer.from_numpy(pp, raw(2101, l * ln)), ln, 61)
            dm = DegRedMask.sample(pp, ln, 62)
            ref = znet.dist_d_pp(pp, net, 2, block_of(ns, ln * eb), block_of(ds, ln * eb), mask_block(dm, ln * eb, DegRedMask), ln, seed=9)
            nr, dr, mr, outs = rows_of(ns, ln * eb), rows_of(ds, ln * eb), mask_rows(dm, ln * eb, DegRedMask), empty_rows(ln * eb)
            per_party(lambda i, pt: pt.d_pp(2, nr[i], dr[i], mr[i], ln, seed=9, out=outs[i]))
            pp.sync()
            checks["d_pp_33"] = np.array_equal(host(outs, ln * eb), ref.to_numpy(np.uint8).reshape(k, ln * eb))
            for grp, is2 in ((ZK_G1, False), (ZK_G2, True)):
                gen_i = BN254.g2 if is2 else BN254.g1
                flat = [gen_i[0][0], gen_i[0][1], gen_i[1][0], gen_i[1][1]] if is2 else list(gen_i)
                gen = pp.fq.encode(flat).reshape(-1)
                w = gen.size * 8
                for ln in (1, 65, 1000):
                    bases = zg.base_points(pp, grp, DeviceBuffer.from_numpy(pp, raw(2200 + ln, n * ln)), n * ln)
                    scal = raw(2300 + ln, n * ln)
                    mm = MsmMask.sample(pp, grp, gen, 70 + ln + int(is2))
                    ref = znet.dist_d_msm(pp, net, 0, grp, block_of(bases, ln * w), block_of(scal, ln * eb), ln,
                                          MsmMask(mm.in_mask[sel], mm.out_mask[sel]))
                    br, sr = rows_of(bases, ln * w), rows_of(scal, ln * eb)
                    got = per_party(lambda i, pt: pt.d_msm(0, grp, br[i], sr[i], ln, mm.in_mask[sel[i]], mm.out_mask[sel[i]]))
                    checks["d_msm_g%d_%d" % (2 if is2 else 1, ln)] = all(same_point(got[i], ref[i], is2) for i in range(k))
            # circom_h at log2_m 6, all seven masks
            log_m = 6
            Lc = (1 << log_m) // l
            qs = [raw(2400 + j, n * Lc) for j in range(3)]
            masks = zg.ProofMasks(pp, log_m, seed=510)
            from zksaas_amd import multigpu as mg
            mct, keep_ = mg.local_masks(pp, masks, log_m, net.first, k, sel)
            ref = znet.dist_circom_h(pp, net, [block_of(x, Lc * eb) for x in qs], log_m, masks=mct, seed=4)
            qr = [rows_of(x, Lc * eb) for x in qs]
            fin = [rows_of(masks.fft[j].in_mask, Lc * eb) for j in range(6)]
            fout = [rows_of(masks.fft[j].out_mask, Lc * eb) for j in range(6)]
            din, dout = rows_of(masks.degred.in_mask, Lc * eb), rows_of(masks.degred.out_mask, Lc * eb)
            hs = empty_rows(Lc * eb)
            cts = []

            def one_h(i, pt):
                mk = zg.Masks()
                for j in range(6):
                    mk.fft_in[j], mk.fft_out[j] = fin[j][i].ptr, fout[j][i].ptr
                mk.degred_in, mk.degred_out = din[i].ptr, dout[i].ptr
                cts.append(mk)
                pt.circom_h([qr[0][i], qr[1][i], qr[2][i]], log_m, masks=mk, seed=4, out=hs[i])
            per_party(one_h)
            pp.sync()
            checks["circom_h_6"] = np.array_equal(host(hs, Lc * eb), ref.to_numpy(np.uint8).reshape(k, Lc * eb))
            # the prover on small_r1cs(): the shares of the rank call, and a proof that verifies
            crs, setup, wit, masks, r, s, wv, got = prover_case(keep="prove")
            lcrs = mg.LocalCrs(pp, crs, net.first, k, sel)
            qap, a_sh, ax_sh = mg.local_witness(pp, wit, net.first, k, sel)
            mct, keep_ = mg.local_masks(pp, masks, wit.log_m, net.first, k, sel)
            ref = znet.dist_prove(pp, net, lcrs.ct, qap, a_sh, ax_sh, r, s, wit.log_m, masks=mct, seed=9)
            checks["prove_shares"] = all(same_point(got[i][0], ref[0][i], False) and same_point(got[i][1], ref[1][i], True) and
                                         same_point(got[i][2], ref[2][i], False) for i in range(k))
            aff, _ = zg.reconstruct(pp, tuple(np.stack([g_[j] for g_ in got]) for j in range(3)), want_bytes=False)
            pvk = zg.PreparedVk(pp, zg.verifying_key(pp, setup))
            checks["proof_verifies"] = zg.verify(pp, pvk, [aff], [[wv[1]]]) == [True]
            checks["wrong_input_fails"] = zg.verify(pp, pvk, [aff], [[(wv[1] + 1) % BN254.r]]) == [False]
            st = net.party_stats()
            rounds = st["rounds"] - stats0["rounds"]
            data["stats"] = st
            checks["rounds_counted"] = rounds == 6 + 3 + 1 + 6 + 1 + 1
            if mode == "staged":
                checks["every_round_staged"] = st["staged"] == st["rounds"] and st["zero_copy"] == 0 and st["bytes_staged"] > 0
            else:
                checks["nothing_staged"] = st["bytes_staged"] == 0 and st["staged"] == 0 and st["zero_copy"] == st["rounds"]

        elif scenario == "ranks":
            # ---- several ranks of k threads each: d_fft at 2^10 and the prover, then d_fft under the all-to-all king
            checks["d_fft_10"] = fft_case(10, False, keep="d_fft_10")
            prover_case(keep="prove")
            checks["prove_ran"] = True
            pp.set_option("king_alltoall", 1)
            checks["d_fft_10_a2a"] = fft_case(10, False, keep="d_fft_10_a2a")
            checks["a2a_used"] = net.stats()["alltoalls"] > 0

        elif scenario == "chan3":
            # ---- three channels in flight: 3 k threads on sids 0, 1, 2 at once against the same calls one after another
            log_m = 10
            Lc = (1 << log_m) // l
            xs = [raw(3000 + sid, n * Lc) for sid in range(3)]
            refs = []
            for sid in range(3):
                b = block_of(xs[sid], Lc * eb)
                znet.dist_d_fft(pp, net, sid, b, FftMask.zero(), False, log_m, seed=20 + sid)
                refs.append(b)
            rows = [rows_of(xs[sid], Lc * eb) for sid in range(3)]
            handles = [[net.party(p_) for p_ in sel] for _ in range(3)]      # a handle per (party, thread)
            fns = [lambda sid=sid, i=i: handles[sid][i].d_fft(sid, rows[sid][i], FftMask.zero(), False, log_m, seed=20 + sid)
                   for sid in range(3) for i in range(k)]
            res, errs = run_threads(fns)
            checks["no_errors"] = all(e is None for e in errs)
            if not checks["no_errors"]:
                checks["errors: " + repr([repr(e) for e in errs if e is not None][:2])] = False
            pp.sync()
            for sid in range(3):
                got = host(rows[sid], Lc * eb)
                checks["sid_%d" % sid] = np.array_equal(got, refs[sid].to_numpy(np.uint8).reshape(k, Lc * eb))
                data["sid_%d" % sid] = {sel[i]: got[i] for i in range(k)}

        elif scenario == "mismatch":
            # ---- party 3 passes log2_m + 1: BAD_INPUT for all eight, party 3 named; the next round on the same net works
            log_m = 6
            Lc = (1 << log_m) // l
            rows = rows_of(raw(4000, n * 2 * Lc), 2 * Lc * eb)          # room for log2_m + 1

            def one(i, pt):
                try:
                    pt.d_fft(0, rows[i], FftMask.zero(), False, log_m + (1 if sel[i] == 3 else 0), seed=3)
                    return None
                except zk.ZkError as e:
                    return (e.code, e.party, str(e))
            got = per_party(one)
            checks["all_bad_input"] = all(g_ is not None and g_[0] == 4 for g_ in got)
            checks["party_3_named"] = all(g_ is not None and g_[1] == 3 and "party 3" in g_[2] for g_ in got)
            checks["next_round_works"] = fft_case(6, False)

        elif scenario == "rehandle":
            # ---- the sequence of a (party, sid) belongs to the party, not to a handle: after two rounds every handle is
            # released and a new one taken (what a host does that makes its net handles per task); then handles of one party
            # take turns; every round equals its rank call
            checks["round_0"] = fft_case(6, False)
            checks["round_1"] = fft_case(6, False, seed=4)
            for pt in parties:
                pt.release()
            parties[:] = [net.party(p_) for p_ in sel]
            checks["round_2_new_handles"] = fft_case(6, False, seed=5)
            older = list(parties)
            parties[:] = [net.party(p_) for p_ in sel]
            checks["round_3_second_handles"] = fft_case(6, False, seed=6)
            spare, parties[:] = list(parties), older
            checks["round_4_first_handles_again"] = fft_case(6, False, seed=7)
            checks["other_channel_starts_at_zero"] = fft_case(6, True, sid=1)
            for pt in spare:
                pt.release()

        elif scenario == "misuse":
            try:
                net.party((sel[-1] + 1) % n if world > 1 else n)
                checks["foreign_party_refused"] = False
            except zk.ZkError as e:
                checks["foreign_party_refused"] = e.code == 4
            # a row that is not 16-byte aligned (world 1: the other seven rows are fine)
            log_m = 6
            Lc = (1 << log_m) // l
            big = DeviceBuffer(pp, n * (Lc * eb + 64))
            rows = [big.view(i * (Lc * eb + 64) + (8 if i == 2 else 0), Lc * eb) for i in range(k)]

            def one(i, pt):
                try:
                    pt.d_fft(0, rows[i], FftMask.zero(), False, log_m, seed=3)
                    return None
                except zk.ZkError as e:
                    return (e.code, str(e))
            got = per_party(one)
            checks["misaligned_row_refused"] = all(g_ is not None and g_[0] == 4 and "aligned" in g_[1] for g_ in got)
            checks["net_still_usable"] = fft_case(6, False)
            # k > 32: a host-mode net of 64 parties on one rank
            big_net = znet.StarNet(None, 0, 1, None, "local", n_parties=64)
            try:
                big_net.party(0)
                checks["k_above_32_refused"] = False
            except zk.ZkError as e:
                checks["k_above_32_refused"] = e.code == 4
            big_net.close()

        elif scenario == "away":
            # ---- four ranks of two threads; party 7 never calls.  First the same thing with the rank call on a net of its
            # own: rank 3 does not call zk_dist_d_fft.  What the rank call gives the other ranks is the reference, whatever
            # it is.  At l = 2, n = 8 it is an ERROR: the six present parties are not more than 2 (t + l - 1) = 6, so the king
            # returns ZK_ERR_PROTOCOL "Not enough shares to reconstruct" (pss.rs:183-186) and the other ranks wait for its
            # scatter in vain (ZK_ERR_NOT_CONNECTED).  The party calls of ranks 0 .. 2 must end in the same way; had the rank
            # call given rows, they would have to give those rows.
            log_m = 10
            Lc = (1 << log_m) // l
            x = raw(5000, n * Lc)
            net_b = znet.StarNet(pp, rank, world, net_ids[1], transport, timeout_ms=timeout_ms)
            ref = None
            if rank != world - 1:
                blk = block_of(x, Lc * eb)
                try:
                    znet.dist_d_fft(pp, net_b, 0, blk, FftMask.zero(), False, log_m, seed=3)
                    pp.sync()
                    ref = ("ok", blk.to_numpy(np.uint8).reshape(k, Lc * eb))
                except zk.ZkError as e:
                    ref = (e.code, str(e).split(" (party")[0])
            rows = rows_of(x, Lc * eb)
            # the ranks leave the failed round at different times (the king at once, the others after their wait for its
            # scatter): bring them into step again, or the king's patience in the next round runs out on THEM
            barrier.wait(timeout=30)

            def one(i, pt):
                if sel[i] == n - 1:
                    return "away"
                t0 = time.monotonic()
                try:
                    pt.d_fft(0, rows[i], FftMask.zero(), False, log_m, seed=3)
                    return ("ok", "", -1, time.monotonic() - t0)
                except zk.ZkError as e:
                    return (e.code, str(e).split(" (party")[0], e.party, time.monotonic() - t0)
            got = per_party(one, limit=30.0)
            pp.sync()
            data["outcome"] = {"rank_call": None if ref is None else ref[0], "party_calls": [g_ if isinstance(g_, str) else g_[0] for g_ in got]}
            if rank == world - 1 and k == 1:
                checks["the_absent_party_is_the_whole_rank"] = got == ["away"]
            elif rank == world - 1:
                g6 = got[0]
                checks["party_6_gets_protocol_naming_7"] = g6[0] == 2 and g6[2] == n - 1
                checks["within_the_deadline"] = 1.5 < g6[3] < 4.0
            elif ref[0] == "ok":
                checks["calls_succeeded"] = all(g_[0] == "ok" for g_ in got)
                checks["rows_of_the_rank_call_without_rank_3"] = np.array_equal(host(rows, Lc * eb), ref[1])
            else:
                checks["the_rank_call's_error %r for both parties, got %r" % (ref, [g_[:2] for g_ in got])] = all(
                    g_[0] == ref[0] and g_[1] == ref[1] for g_ in got)
            net_b.close()
        else:
            raise ValueError("unknown scenario " + scenario)

        for pt in parties:
            pt.release()
        q.put((rank, all(checks.values()), repr(checks), data))
        net.close()
    except BaseException as e:      # noqa: BLE001
        import traceback
        q.put((rank, False, traceback.format_exc()[-2500:] + repr(e), {}))
