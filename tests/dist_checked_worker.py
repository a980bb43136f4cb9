"""Worker of tests/test_gpu_dist_checked.py: one rank of the star network running the CHECKED king rounds
(zk_dist_d_fft_checked, zk_dist_d_ifft_checked, zk_dist_deg_red_checked, zk_dist_circom_h_checked) over shared memory,
BN254, l = 2, n = 8, replayable randomness.  Every rank deals the SAME seeded inputs, wrong rows included, runs the
single-device checked call on its own context as the expectation, and sends the parent (rank, verdict, details, report): per
checked call its status and errpos bytes, its summary, and what the single-device call reported -- the parent combines the
ranks' parts (tests/test_gpu_dist_checked.py)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 5                                     # the coset shift of the d_ifft cases
A2A_LOG_M = {2: 8, 4: 9, 8: 10}           # the smallest m at which a2a_plan applies to d_fft: m / l >= 64 * world columns


def run(rank, world, net_id, scenario, q, transport="shm"):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        import zksaas_amd as zk
        from zksaas_amd import groth16 as zg
        from zksaas_amd import multigpu as mg
        from zksaas_amd import net as znet
        from zksaas_amd.api import DegRedMask, DeviceBuffer, FftMask

        a2a = scenario.endswith("_a2a")
        if a2a:
            scenario = scenario[:-4]
        late_log_m = 0                               # "late11": the late scenario at log2_m = 11
        if scenario.startswith("late"):
            late_log_m, scenario = int(scenario[4:] or 0), "late"
        zk.api.DEFAULT_OPTIONS["rng_replay"] = 1     # a spawned process: the parent's conftest does not reach here
        pp = zk.PackedSharingParams("bn254", 2)
        if a2a:
            pp.set_option("king_alltoall", 1)
        net = znet.StarNet(pp, rank, world, net_id, transport, timeout_ms=60000)
        k, n, l = net.k, pp.n, pp.l
        sel = list(net.parties)
        eb = pp.fr.nbytes
        if scenario == "late":
            # all-to-all: 13 gives 64 granules of 64 chunks over the seven present ranks (ranges of 640 and one of 256), 11 gives
            # 16 granules: five ranges of 192 chunks, one of 64 and one EMPTY
            log_m = late_log_m or (13 if a2a else 10)
        elif scenario == "circom_h" or not a2a:
            log_m = 10
        else:
            log_m = A2A_LOG_M[world]
        Lc = (1 << log_m) // l

        def raw(seed, *shape):
            a = np.random.default_rng(seed).integers(0, 1 << 62, size=shape + (4,), dtype=np.uint64)
            a[..., 3] &= np.uint64((1 << 60) - 1)
            return a

        def dev(arr):
            return DeviceBuffer.from_numpy(pp, np.ascontiguousarray(arr))

        def honest(seed):                 # packed shares [n][Lc][4] of random secrets: every chunk a word of degree < 2l
            return pp.pack(dev(raw(seed, Lc * l)), Lc, seed=seed).to_numpy().reshape(n, Lc, 4).copy()

        def products(seed):               # a * b element by element: words of degree 4l - 2, the dimension of deg_red
            a, b, zero = dev(honest(seed)), dev(honest(seed + 1)), dev(np.zeros((n * Lc, 4), np.uint64))
            out = pp.alloc_fr(n * Lc)
            pp._check(pp.lib.zk_vec_mul_sub(pp.h, out.ptr, a.ptr, b.ptr, zero.ptr, n * Lc, None))
            return out.to_numpy().reshape(n, Lc, 4).copy()

        def lie(rows, parties, seed):     # the whole row of every listed party replaced
            cur = rows.copy()
            for p_ in parties:
                cur[p_] = raw(seed + p_, Lc)
            return cur

        def loc(arr):
            return dev(arr.reshape(n, Lc, 4)[sel])

        def lmask(m, cls):
            return cls(mg.rows_of(pp, m.in_mask, sel, Lc * eb), mg.rows_of(pp, m.out_mask, sel, Lc * eb))

        def mine_of(full_dev):            # this rank's rows of a single-device result
            return full_dev.to_numpy().reshape(n, Lc, 4)[sel]

        def got(local_dev):
            return local_dev.to_numpy().reshape(k, Lc, 4)

        checks, report = {}, {}

        def record(name, rep, want):
            """this rank's part of the report and what the single-device call reported (want: a RobustUnpack or None)"""
            report[name] = {
                "status": rep.status_host().copy(), "errpos": rep.errpos_host().copy(), "summaries": rep.summaries,
                "want_status": None if want is None else want.status_host().copy(),
                "want_errpos": None if want is None else want.errpos_host().copy(),
                "want_summaries": None if want is None else want.summaries}

        # the liars of a scenario: whole ranks
        liar_rank = {"honest": None, "circom_h": None, "liar": {8: 3, 4: 1}.get(world), "beyond": 1, "late": 2}[scenario]
        liars = [] if liar_rank is None else list(range(liar_rank * k, liar_rank * k + k))
        present = list(range(n - k)) if scenario == "late" else None        # the last rank enters late

        if scenario == "circom_h":
            # ---- zk_dist_circom_h_checked: a liar in round 1 (a wrong qap_a row), all seven masks on
            qs = [honest(700 + 10 * i) for i in range(3)]
            wrong = [lie(qs[0], [3], 740), qs[1], qs[2]]
            masks = zg.ProofMasks(pp, log_m, seed=500)
            mct, keep = mg.local_masks(pp, masks, log_m, net.first, k, sel)
            h_honest = znet.dist_circom_h(pp, net, [loc(x) for x in qs], log_m, masks=mct, seed=4)
            h_ref, want = zk.api.circom_h(pp, [dev(x) for x in wrong], masks=masks, seed=4, check=True, log2_m=log_m)
            h, rep = znet.dist_circom_h_checked(pp, net, [loc(x) for x in wrong], log_m, masks=mct, seed=4)
            pp.sync()
            checks["h_equals_the_honest_dist_circom_h"] = np.array_equal(got(h), got(h_honest))
            checks["h_equals_circom_h_checked"] = np.array_equal(got(h), mine_of(h_ref))
            checks["summaries_equal_the_single_device_report"] = rep.summaries == want.summaries
            checks["item_0_names_the_party"] = want.summaries[0] == [0, Lc, 0] + [Lc if p_ == 3 else 0 for p_ in range(n)]
            checks["other_items_clean"] = all(want.summaries[i] == [Lc, 0, 0] + [0] * n for i in range(1, 7))
            record("circom_h", rep, want)
            checks["king_mode"] = (net.stats()["alltoalls"] > 0) == a2a
            q.put((rank, all(checks.values()), repr(checks), report))
            net.close()
            return

        # ---- inputs, dealt alike on every rank before the first round
        x_fft = honest(100)
        x_deg = products(200)
        bad_fft = lie(x_fft, liars, 300) if liars else x_fft
        bad_deg = lie(x_deg, liars, 400) if liars else x_deg
        fft_cases = [("d_fft", False, False, 11), ("d_ifft", True, True, 12)]
        fmasks = {name: FftMask.sample(pp, rearr, G if inv else None, int(inv), log_m, 40 + sd) for name, inv, rearr, sd in fft_cases}
        dmask = DegRedMask.sample(pp, Lc, 50)

        def single_fft(rows, name, inv, rearr, sd, check, parties=None):
            buf = dev(rows)
            fn = zk.d_ifft if inv else zk.d_fft
            kw = {"g": G} if inv else {}
            if parties is not None:
                kw["parties"] = parties
            r = fn(pp, buf, fmasks[name], rearr, log_m, seed=sd, check=check, **kw)
            return buf, (r if check else None)

        def dist_fft(rows, name, inv, rearr, sd, check, sid):
            buf = loc(rows)
            lm = lmask(fmasks[name], FftMask)
            if inv:
                fn = znet.dist_d_ifft_checked if check else znet.dist_d_ifft
                r = fn(pp, net, sid, buf, lm, rearr, log_m, g=G, seed=sd)
            else:
                fn = znet.dist_d_fft_checked if check else znet.dist_d_fft
                r = fn(pp, net, sid, buf, lm, rearr, log_m, seed=sd)
            return buf, (r[1] if check else None)

        if scenario == "late":
            # a warm-up round brings the ranks into step; then the king's patience is cut, the last rank comes late and is
            # left out, rank 2 lies: the list repair (seven parties, cap 1) corrects every chunk
            znet.dist_d_fft(pp, net, 0, loc(x_fft), FftMask.zero(), False, log_m, seed=1)
            pp.sync()
            net.lib.zk_net_set_timeout_ms(net.h, 1000)
            name, inv, rearr, sd = fft_cases[0]
            if rank == world - 1:
                time.sleep(2.5)
                try:
                    dist_fft(bad_fft, name, inv, rearr, sd, True, 0)
                    q.put((rank, False, "late rank was admitted", {}))
                except zk.ZkError as e:
                    q.put((rank, e.code == 2, "code %d party %d" % (e.code, e.party), {}))
                net.close()
                return
            buf, rep = dist_fft(bad_fft, name, inv, rearr, sd, True, 0)
            ref, want = single_fft(bad_fft, name, inv, rearr, sd, True, parties=present)
            pp.sync()
            checks["d_fft_equals_d_fft_checked_parties"] = np.array_equal(got(buf), mine_of(ref))
            checks["d_fft_summary"] = rep.summary == want.summary == [0, Lc, 0] + [Lc if p_ == 2 else 0 for p_ in range(n)]
            record("d_fft", rep, want)
            # deg_red with the rank absent: NOT CHECKED -- the all-zero row; the output is the unchecked round's
            dbuf, drep = znet.dist_deg_red_checked(pp, net, 1, loc(bad_deg), lmask(dmask, DegRedMask), Lc, seed=13)
            ubuf = znet.dist_deg_red(pp, net, 1, loc(bad_deg), lmask(dmask, DegRedMask), Lc, seed=13)
            pp.sync()
            checks["deg_red_equals_the_unchecked_round"] = np.array_equal(got(dbuf), got(ubuf))
            checks["deg_red_not_checked"] = (drep.summary == [0] * (3 + n) and not drep.status_host().any()
                                             and not drep.errpos_host().any())
            checks["king_mode"] = (net.stats()["alltoalls"] > 0) == a2a
            q.put((rank, all(checks.values()), repr(checks), report))
            net.close()
            return

        for i, (name, inv, rearr, sd) in enumerate(fft_cases):
            buf, rep = dist_fft(bad_fft, name, inv, rearr, sd, True, i)
            ref, want = single_fft(bad_fft, name, inv, rearr, sd, True)
            pp.sync()
            checks[name + "_equals_the_single_device_checked_call"] = np.array_equal(got(buf), mine_of(ref))
            checks[name + "_summary_is_the_single_device_summary"] = rep.summary == want.summary
            record(name, rep, want)
            if scenario == "honest" or scenario == "beyond":
                # honest: the checked round changes nothing; beyond the cap: the shares went to the king as received
                ubuf, _ = dist_fft(bad_fft, name, inv, rearr, sd, False, i)
                pp.sync()
                checks[name + "_equals_the_unchecked_round"] = np.array_equal(got(buf), got(ubuf))
            if scenario == "liar":
                href, _ = single_fft(x_fft, name, inv, rearr, sd, False)
                pp.sync()
                checks[name + "_equals_the_honest_run"] = np.array_equal(got(buf), mine_of(href))
        # deg_red: detection only -- with a liar every chunk fails and the word goes to the king as received
        dbuf, drep = znet.dist_deg_red_checked(pp, net, 2, loc(bad_deg), lmask(dmask, DegRedMask), Lc, seed=13)
        full = dev(bad_deg)
        dwant = zk.deg_red(pp, full, dmask, Lc, seed=13, check=True)
        ubuf = znet.dist_deg_red(pp, net, 2, loc(bad_deg), lmask(dmask, DegRedMask), Lc, seed=13)
        pp.sync()
        checks["deg_red_equals_the_single_device_checked_call"] = np.array_equal(got(dbuf), mine_of(full))
        checks["deg_red_equals_the_unchecked_round"] = np.array_equal(got(dbuf), got(ubuf))
        checks["deg_red_summary_is_the_single_device_summary"] = drep.summary == dwant.summary
        record("deg_red", drep, dwant)
        if scenario == "honest":
            # circom_h on honest words: the unchecked h, seven clean items
            qs = [honest(700 + 10 * i) for i in range(3)]
            masks = zg.ProofMasks(pp, log_m, seed=500)
            mct, keep = mg.local_masks(pp, masks, log_m, net.first, k, sel)
            h_un = znet.dist_circom_h(pp, net, [loc(x) for x in qs], log_m, masks=mct, seed=4)
            h, hrep = znet.dist_circom_h_checked(pp, net, [loc(x) for x in qs], log_m, masks=mct, seed=4)
            h_ref, hwant = zk.api.circom_h(pp, [dev(x) for x in qs], masks=masks, seed=4, check=True, log2_m=log_m)
            pp.sync()
            checks["circom_h_equals_the_unchecked_round"] = np.array_equal(got(h), got(h_un))
            checks["circom_h_equals_circom_h_checked"] = np.array_equal(got(h), mine_of(h_ref))
            checks["circom_h_summaries"] = hrep.summaries == hwant.summaries == [[Lc, 0, 0] + [0] * n] * 7
            record("circom_h", hrep, hwant)
        if world > 1:
            checks["king_mode"] = (net.stats()["alltoalls"] > 0) == a2a
        q.put((rank, all(checks.values()), repr(checks), report))
        net.close()
    except Exception as e:      # noqa: BLE001
        import traceback
        q.put((rank, False, traceback.format_exc()[-2500:] + repr(e), {}))
