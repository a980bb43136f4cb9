"""The checked king rounds on the star network (zk_dist_d_fft_checked, zk_dist_d_ifft_checked, zk_dist_deg_red_checked,
zk_dist_circom_h_checked over zk_net_*): the word a king RECEIVES from the other ranks is repaired before the king reads it.
Ranks are processes sharing this box's one GPU through the shared-memory transport; BN254, l = 2, n = 8, replayable
randomness (tests/dist_checked_worker.py).  Each scenario in the star and in the all-to-all king mode:
  honest      worlds 1 (local), 2, 4, 8: rows bit for bit the unchecked round's, every status 0, summary [chunks, 0, 0, ..]
  liar        world 8: rank 3's vector replaced (k = 1); world 4: both rows of rank 1 (cap = l = 2 wrong shares): every chunk
              corrected, the output the honest run's, the party named
  beyond      world 2: all four rows of rank 1 wrong: every chunk fails, the output the unchecked round's, no error
  late        world 8, a rank left out and a liar among the seven: the list repair corrects every chunk; the all-to-all leg at
              log2_m = 13 (uneven ranges) and at log2_m = 11 (uneven ranges, one of them EMPTY)
  circom_h    world 8: a wrong qap_a row; item 0 names the party
The parent combines what the ranks report: the OR of their status / errpos parts is the single-device report, each chunk is
reported by exactly one rank (rank 0 in the star), and the summary is the single-device one on EVERY rank.
The last tests run the range form of the repair alone, in this process (zk_pss_repair_range)."""
import multiprocessing as mp
import os
import queue
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300.0            # seconds a scenario may take, start of the workers included
N, L = 8, 2


def _spawn(world, scenario, transport="shm"):
    """-> {rank: report}; fails unless every rank sends a passing verdict within the limit.  Workers that are left when the
    verdicts are in, or when the scenario has failed, are ended; nothing is tried again."""
    assert world <= 8
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_checked_worker
    from zksaas_amd.net import StarNet
    net_id = StarNet.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=dist_checked_worker.run, args=(r, world, net_id, scenario, q, transport)) for r in range(world)]
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
    assert not bad, bad
    return {r[0]: r[3] for r in results}


def _combine(reports, name, a2a, ranks=None):
    """the ranks' parts of one call's report -> (status, errpos, summaries), with the assertions that hold in every scenario"""
    ranks = sorted(reports) if ranks is None else ranks
    parts = [reports[r][name] for r in ranks]
    want = parts[0]
    status = np.zeros_like(parts[0]["status"])
    errpos = np.zeros_like(parts[0]["errpos"])
    owners = np.zeros(len(status), np.int32)
    for r, p in zip(ranks, parts):
        assert p["summaries"] == want["want_summaries"], (name, r, p["summaries"])       # complete and identical on every rank
        assert p["want_summaries"] == want["want_summaries"]
        # a rank reports a chunk only with a nonzero status; errpos only where it reports
        assert not (p["errpos"][p["status"] == 0]).any(), (name, r)
        owners += p["status"] != 0
        status |= p["status"]
        errpos |= p["errpos"]
        if not a2a and r != 0:
            assert not p["status"].any() and not p["errpos"].any(), (name, r)            # the star: rank 0 is the only king
    assert (owners <= 1).all(), name                                                     # each chunk reported by one rank
    assert np.array_equal(status, want["want_status"]) and np.array_equal(errpos, want["want_errpos"]), name
    if a2a and len(ranks) > 1 and status.any():
        assert sum(1 for p in parts if p["status"].any()) > 1, name                      # the ranges really are spread out
    return status, errpos, want["want_summaries"]


def _chunks(world, scenario, a2a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_checked_worker import A2A_LOG_M
    if scenario.startswith("late"):
        log_m = int(scenario[4:] or (13 if a2a else 10))
    else:
        log_m = A2A_LOG_M[world] if a2a and scenario != "circom_h" else 10
    return (1 << log_m) // L


def _name(scenario, a2a):
    return scenario + ("_a2a" if a2a else "")


# ---------------------------------------------------------------- 1. honest
@pytest.mark.parametrize("world,a2a", [(1, False), (2, False), (4, False), (8, False), (2, True), (4, True), (8, True)])
def test_honest_rounds_change_nothing_and_report_clean(world, a2a):
    reports = _spawn(world, _name("honest", a2a), "local" if world == 1 else "shm")
    lc = _chunks(world, "honest", a2a)
    for name in ("d_fft", "d_ifft", "deg_red"):
        status, errpos, sums = _combine(reports, name, a2a)
        assert len(status) == lc and not status.any() and not errpos.any()
        assert sums == [[lc, 0, 0] + [0] * N]
    status, errpos, sums = _combine(reports, "circom_h", a2a)
    assert len(status) == 7 * lc and not status.any() and sums == [[lc, 0, 0] + [0] * N] * 7


# ---------------------------------------------------------------- 2. / 3. one lying rank
@pytest.mark.parametrize("world,a2a", [(8, False), (8, True), (4, False), (4, True)])
def test_one_lying_rank_is_corrected_and_named(world, a2a):
    reports = _spawn(world, _name("liar", a2a))
    lc = _chunks(world, "liar", a2a)
    liars = [3] if world == 8 else [2, 3]             # rank 3 of 8; both rows of rank 1 of 4: cap = l wrong shares
    bits = sum(1 << p for p in liars)
    for name in ("d_fft", "d_ifft"):
        status, errpos, sums = _combine(reports, name, a2a)
        assert len(status) == lc and (status == 1).all() and (errpos == bits).all()
        assert sums == [[0, lc, 0] + [lc if p in liars else 0 for p in range(N)]]
    # deg_red only detects: every chunk fails, nobody is named
    status, errpos, sums = _combine(reports, "deg_red", a2a)
    assert (status == 2).all() and not errpos.any() and sums == [[0, 0, lc] + [0] * N]


# ---------------------------------------------------------------- 4. beyond the cap
@pytest.mark.parametrize("a2a", [False, True])
def test_more_liars_than_the_cap_fail_every_chunk_without_an_error(a2a):
    reports = _spawn(2, _name("beyond", a2a))
    lc = _chunks(2, "beyond", a2a)
    for name in ("d_fft", "d_ifft", "deg_red"):
        status, errpos, sums = _combine(reports, name, a2a)
        assert len(status) == lc and (status == 2).all() and not errpos.any()
        assert sums[0][2] == lc and sums == [[0, 0, lc] + [0] * N]


# ---------------------------------------------------------------- 5. a late rank and a liar
@pytest.mark.parametrize("scenario,a2a", [("late", False), ("late", True), ("late11", True)], ids=["star", "a2a_2p13", "a2a_2p11"])
def test_a_late_rank_is_left_out_and_the_liar_among_the_rest_is_corrected(scenario, a2a):
    """all-to-all, seven ranks present, granules of 64 chunks: at log2_m = 13 the 64 granules give ranges of 640 chunks and one
    of 256; at log2_m = 11 the 16 granules give seg = 192: five ranges of 192, one of 64 and one EMPTY -- that rank repairs
    nothing, reports nothing, and still holds the whole word's summary (_combine asserts it for every rank)"""
    reports = _spawn(8, _name(scenario, a2a))
    lc = _chunks(8, scenario, a2a)
    present = list(range(7))
    status, errpos, sums = _combine(reports, "d_fft", a2a, present)
    assert len(status) == lc and (status == 1).all() and (errpos == 1 << 2).all()
    assert sums == [[0, lc, 0] + [lc if p == 2 else 0 for p in range(N)]]
    if a2a:
        owned = [int((reports[r]["d_fft"]["status"] != 0).sum()) for r in present]
        assert owned == ([640] * 6 + [256] if lc == 4096 else [192] * 5 + [64, 0]), owned
        assert sum(owned) == lc


# ---------------------------------------------------------------- 6. circom_h
@pytest.mark.parametrize("a2a", [False, True])
def test_circom_h_checked_names_the_liar_of_round_one(a2a):
    reports = _spawn(8, _name("circom_h", a2a))
    lc = _chunks(8, "circom_h", a2a)
    status, errpos, sums = _combine(reports, "circom_h", a2a)
    status, errpos = status.reshape(7, lc), errpos.reshape(7, lc)
    assert (status[0] == 1).all() and (errpos[0] == 1 << 3).all()
    assert not status[1:].any() and not errpos[1:].any()
    assert sums[0] == [0, lc, 0] + [lc if p == 3 else 0 for p in range(N)] and sums[1:] == [[lc, 0, 0] + [0] * N] * 6


# ---------------------------------------------------------------- 7. the range form alone
def _raw(rng, *shape):
    a = rng.integers(0, 1 << 62, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


def _range_call(pp, zk, rows, parties, stride, cnt, ln, base, shift, dimension, fill=0xEE):
    """zk_pss_repair_range on a copy of `rows` [np][stride][4]; status / errpos pre-filled so that untouched entries show"""
    import ctypes as C
    buf = zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(rows))
    status = zk.DeviceBuffer.from_numpy(pp, np.full(ln, fill, np.uint8))
    errpos = zk.DeviceBuffer.from_numpy(pp, np.full(ln, 0xEEEEEEEE, np.uint32))
    summary = zk.DeviceBuffer.from_numpy(pp, np.full(3 + pp.n, 77, np.uint64))
    arr = None if parties is None else (C.c_uint32 * len(parties))(*parties)
    pp._check(pp.lib.zk_pss_repair_range(pp.h, buf.ptr, arr, len(rows), stride, cnt, ln, base, shift, dimension, status.ptr,
                                         errpos.ptr, summary.ptr, None))
    pp.sync()
    return (buf.to_numpy().reshape(rows.shape), status.to_numpy(np.uint8), errpos.to_numpy(np.uint32),
            [int(v) for v in summary.to_numpy(np.uint64)])


@pytest.mark.parametrize("parties", [None, [0, 1, 2, 4, 5, 6, 7]], ids=["all", "list"])
def test_range_form_over_the_whole_word_is_repair_parties(parties):
    import zksaas_amd as zk
    from gpu_util import ctx
    pp = ctx("bn254", 2)
    ln = 700                                   # three workgroups of the scan, the last one partial
    rng = np.random.default_rng(5)
    word = pp.pack(zk.DeviceBuffer.from_numpy(pp, _raw(rng, ln * 2)), ln, seed=9).to_numpy().reshape(8, ln, 4).copy()
    word[1, ::3] = _raw(rng, len(range(0, ln, 3)))                # one wrong share: corrected
    word[5, 100:200] = _raw(rng, 100)                             # a second one in some chunks
    word[6, 150:160] = _raw(rng, 10)                              # three wrong shares: beyond the cap of either list
    rows = word if parties is None else word[parties]
    r = pp.repair(zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(rows)), ln, parties=parties)
    pp.sync()
    got_rows, status, errpos, summary = _range_call(pp, zk, rows, parties, ln, ln, ln, 0, 0, 4)
    assert set(r.status_host().tolist()) == {0, 1, 2}
    assert np.array_equal(status, r.status_host()) and np.array_equal(errpos, r.errpos_host()) and summary == r.summary
    assert np.array_equal(got_rows, r.out.to_numpy().reshape(rows.shape))           # the shares written, byte for byte


@pytest.mark.parametrize("parties", [None, [0, 1, 2, 3, 4, 5, 7]], ids=["all", "list"])
def test_range_form_of_a_block_with_padding(parties):
    """a rank's [np][seg] block under the all-to-all king of d_fft: cnt < seg valid columns, shift 1, a nonzero base"""
    import zksaas_amd as zk
    from gpu_util import ctx
    pp = ctx("bn254", 2)
    ln, seg, cnt, base, shift = 1024, 384, 256, 768, 1          # the last of three ranges: chunks 767 .. 1022
    rng = np.random.default_rng(6)
    word = pp.pack(zk.DeviceBuffer.from_numpy(pp, _raw(rng, ln * 2)), ln, seed=10).to_numpy().reshape(8, ln, 4).copy()
    chunk_of = [(base + c + ln - shift) % ln for c in range(cnt)]
    word[2, 800:900] = _raw(rng, 100)                             # a wrong share in the chunks 800 .. 899: corrected, party 2
    word[0, 767] = _raw(rng, 1)[0]                                # the first column of the range
    word[4, 0:767] = _raw(rng, 767)                               # wrong shares OUTSIDE the range: never seen
    rows = word if parties is None else word[parties]
    np_ = len(rows)
    block = _raw(rng, np_, seg)                                   # padding: random elements, no codewords
    block[:, :cnt] = rows[:, chunk_of]
    want = pp.repair(zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(rows)), ln, parties=parties)
    pp.sync()
    ws, we = want.status_host(), want.errpos_host()
    fixed = want.out.to_numpy().reshape(rows.shape)
    got_block, status, errpos, summary = _range_call(pp, zk, block, parties, seg, cnt, ln, base, shift, 4)
    assert np.array_equal(got_block[:, cnt:], block[:, cnt:])                       # the padding keeps its bytes
    assert np.array_equal(got_block[:, :cnt], fixed[:, chunk_of])                   # the valid columns are repaired
    inside = np.zeros(ln, bool)
    inside[chunk_of] = True
    assert np.array_equal(status[inside], ws[inside]) and np.array_equal(errpos[inside], we[inside])
    assert (status[~inside] == 0xEE).all() and (errpos[~inside] == 0xEEEEEEEE).all()   # written at the mapped chunks only
    assert (ws[800:900] == 1).all() and (we[800:900] == 1 << 2).all() and ws[767] == 1 and we[767] == 1
    assert summary == [cnt - 101, 101, 0, 1, 0, 100, 0, 0, 0, 0, 0]
    # an empty range: nothing is read or written but the summary, which is cleared
    got_block, status, errpos, summary = _range_call(pp, zk, block, parties, seg, 0, ln, 0, shift, 4)
    assert np.array_equal(got_block, block) and (status == 0xEE).all() and summary == [0] * 11
    # refusals write nothing
    import ctypes as C
    buf = zk.DeviceBuffer.from_numpy(pp, np.ascontiguousarray(block))
    st = zk.DeviceBuffer.from_numpy(pp, np.full(ln, 0xEE, np.uint8))
    arr = None if parties is None else (C.c_uint32 * len(parties))(*parties)
    for stride_, cnt_, base_ in ((cnt - 1, cnt, base), (seg, ln + 1, base), (seg, cnt, ln)):
        assert pp.lib.zk_pss_repair_range(pp.h, buf.ptr, arr, np_, stride_, cnt_, ln, base_, shift, 4, st.ptr, None, None, None) == 4
    assert np.array_equal(buf.to_numpy().reshape(block.shape), block) and (st.to_numpy(np.uint8) == 0xEE).all()
