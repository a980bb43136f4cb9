"""The per-party entry points (zk_party_*: one caller per party, a rendezvous per rank and channel, include/zksaas.h) on the
GPU.  BN254, l = 2, n = 8, replayable randomness; the net's timeout is at most 5 s everywhere; every party is a host thread
that is joined with a deadline (tests/party_worker.py), every scenario a set of at most 8 rank processes under a time limit
of its own, as in tests/test_gpu_dist_checked.py.
  1  world 1, eight threads, separately allocated rows: every call equals its rank call, every round is staged
  2  the same with rows carved from one block: equal results, zero bytes staged
  3  two shared-memory ranks of four threads: d_fft at 2^10 and the prover equal case 1's; d_fft again under king_alltoall
  4  three channels in flight, 24 threads at world 1; again on two ranks
  5  a mismatching party: BAD_INPUT for all eight, the party named, the net still usable
  6  a party that stays away (four ranks of two threads, 2 s timeout): its rank fails with PROTOCOL naming it, the other
     ranks end exactly as zk_dist_d_fft ends in the same test when rank 3 does not call -- at l = 2 that is the king's
     "Not enough shares to reconstruct" (six parties present, seven needed), so no rows exist to compare
  7  misuse: a foreign party, a misaligned row, k > 32
  8  handles released and taken again after some rounds, two handles of a party taking turns"""
import functools
import multiprocessing as mp
import os
import queue
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240.0            # seconds a scenario may take, start of the workers included


def _spawn(world, scenario):
    """-> {rank: data}; fails unless every rank sends a passing verdict within the limit.  Workers that are left when the
    verdicts are in, or when the scenario has failed, are ended; nothing is tried again."""
    assert world <= 8
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import party_worker
    from zksaas_amd.net import StarNet
    net_ids = (StarNet.unique_id(), StarNet.unique_id())
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    barrier = ctx.Barrier(world)
    procs = [ctx.Process(target=party_worker.run, args=(r, world, net_ids, scenario, q, "local" if world == 1 else "shm", barrier))
             for r in range(world)]
    deadline = time.monotonic() + LIMIT
    results = []
    try:
        for p in procs:
            p.start()
        while len(results) < world:
            left = deadline - time.monotonic()
            assert left > 0, "scenario %s: %d of %d ranks answered within %d s" % (scenario, len(results), world, LIMIT)
            try:
                results.append(q.get(timeout=min(left, 2.0)))
            except queue.Empty:
                died = [(i, p.exitcode) for i, p in enumerate(procs) if p.exitcode not in (None, 0)]
                assert not died, "scenario %s: workers died (rank, exit code): %r" % (scenario, died)
    finally:
        for p in procs:
            p.join(timeout=0 if len(results) < world else 30)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
            if p.is_alive():
                p.kill()
    bad = [(r[0], r[2]) for r in results if not r[1]]
    for rank, details in bad:
        print("rank %d: %s" % (rank, details))           # (the assertion's own text is cut short)
    assert not bad, bad
    return {r[0]: r[3] for r in results}


@functools.lru_cache(maxsize=None)
def _world1(scenario):
    """the world-1 scenarios other tests compare with: run once, never modified"""
    return _spawn(1, scenario)[0]


def _by_party(reports, name):
    out = {}
    for data in reports.values():
        out.update(data[name])
    assert sorted(out) == list(range(8)), (name, sorted(out))
    return out


def test_eight_threads_with_separate_rows_equal_the_rank_calls_and_every_round_is_staged():
    data = _world1("staged")
    st = data["stats"]
    assert st["rounds"] == 18 and st["staged"] == 18 and st["zero_copy"] == 0 and st["bytes_staged"] > 0, st


def test_rows_carved_from_one_block_give_the_same_results_with_nothing_staged():
    block, staged = _world1("block"), _world1("staged")
    st = block["stats"]
    assert st["rounds"] == 18 and st["zero_copy"] == 18 and st["staged"] == 0 and st["bytes_staged"] == 0, st
    for p in range(8):
        assert np.array_equal(block["d_fft_10"][p], staged["d_fft_10"][p])


def test_two_ranks_of_four_threads_equal_one_rank_of_eight():
    from gpu_util import ctx, dec_jacobian
    from oracle.curve import g1, g2
    from oracle.params import BN254
    one = _world1("staged")
    reports = _spawn(2, "ranks")
    for name in ("d_fft_10", "d_fft_10_a2a"):
        rows = _by_party(reports, name)
        for p in range(8):
            assert np.array_equal(rows[p], one["d_fft_10"][p]), (name, p)
    pp = ctx("bn254", 2)
    G1, G2 = g1(BN254), g2(BN254)
    proofs = _by_party(reports, "prove")
    for p in range(8):
        for j, (G, is2) in enumerate(((G1, False), (G2, True), (G1, False))):
            assert G.eq(dec_jacobian(pp, proofs[p][j], is2), dec_jacobian(pp, one["prove"][p][j], is2)), (p, j)


@pytest.mark.parametrize("world", [1, 2])
def test_three_channels_in_flight_equal_the_calls_one_after_another(world):
    reports = _spawn(world, "chan3")
    if world == 2:
        one = _world1("chan3")
        for sid in range(3):
            rows = _by_party(reports, "sid_%d" % sid)
            for p in range(8):
                assert np.array_equal(rows[p], one["sid_%d" % sid][p]), (sid, p)


def test_a_mismatching_party_is_bad_input_for_all_eight_and_the_net_stays_usable():
    _spawn(1, "mismatch")


def test_a_party_that_stays_away_fails_its_rank_and_the_other_ranks_end_as_with_the_rank_call():
    reports = _spawn(4, "away")
    assert reports[3]["outcome"]["party_calls"] == [2, "away"]
    for r in range(3):
        o = reports[r]["outcome"]
        assert o["party_calls"] == [o["rank_call"]] * 2, (r, o)


def test_eight_ranks_with_party_7_away_give_the_rows_of_the_rank_call_without_it():
    """beyond the issue's case 6, whose rank call has no rows to give at l = 2: with one party per rank seven parties remain,
    which suffice (pss.rs:183-186), so here the ROWS of zk_dist_d_fft without rank 7 are what the party calls must give"""
    reports = _spawn(8, "away")
    assert reports[7]["outcome"]["party_calls"] == ["away"]
    for r in range(7):
        assert reports[r]["outcome"] == {"rank_call": "ok", "party_calls": ["ok"]}, (r, reports[r]["outcome"])


def test_a_new_handle_for_a_party_continues_where_the_last_one_stopped():
    _spawn(1, "rehandle")


def test_misuse_is_bad_input():
    _spawn(1, "misuse")
