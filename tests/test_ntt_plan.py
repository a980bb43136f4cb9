"""csrc/ntt.hpp's make_ntt_plan is host code: the pass plan of fft1 is checked on the CPU for every (log_n, tile bits) the
engine can pass (tests/native/ntt_plan_host_test.cpp), every plan is compared with the plain-Python restatement in
tests/ntt_sizes.py, and for log_n <= 16 the kernel's own index formula, restated with numpy, shows that the tiles of each
pass partition [0, n) and that every butterfly of the pass stays inside one tile."""
import os
import subprocess

import numpy as np
import pytest

import ntt_sizes as ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"

REFUSED_LINES = []          # the native program's "refused k tb" lines (sizes outside the planner's domain)
# the (k, tb) pairs the engine can pass (fft1_tiled): the small tile from its own size up to 2^14, the large one above
ENGINE_PAIRS = [(k, 8) for k in range(8, 15)] + [(k, 11) for k in range(15, 39)]


def _native_plans():
    out = os.path.join(ROOT, "tests", "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "ntt_plan_host_test")
    r = subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "zk-saas_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "ntt_plan_host_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 violations", r.stdout[-4000:]
    plans = {}
    REFUSED_LINES[:] = [ln for ln in lines if ln.startswith("refused ")]
    for ln in lines:
        if not ln.startswith("plan "):
            continue
        f = list(map(int, ln.split()[1:]))
        k, tb, npass = f[:3]
        assert len(f) == 3 + 3 * npass, ln
        plans[(k, tb)] = [tuple(f[3 + 3 * i:6 + 3 * i]) for i in range(npass)]
    assert lines[-2] == "plans %d" % len(plans)
    return plans


def test_ntt_plan_conditions_hold_and_every_plan_equals_the_python_restatement():
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found")
    plans = _native_plans()
    assert sorted(plans) == sorted(ENGINE_PAIRS)
    for (k, tb), got in plans.items():
        assert ns.tile_bits(k) == tb
        assert got == ns.plan(k, tb), (k, tb)
    # a few rows of the table in docs/ntt_size_tests.md, written out by hand
    assert plans[(8, 8)] == [(0, 8, 0)]
    assert plans[(9, 8)] == [(0, 5, 0), (5, 9, 4)]
    assert plans[(14, 8)] == [(0, 8, 0), (8, 14, 2)]
    assert plans[(15, 11)] == [(0, 8, 0), (8, 15, 4)]
    assert plans[(20, 11)] == [(0, 11, 0), (11, 20, 2)]
    assert plans[(21, 11)] == [(0, 7, 0), (7, 14, 4), (14, 21, 4)]
    assert plans[(29, 11)] == [(0, 11, 0), (11, 20, 2), (20, 29, 2)]
    assert [len(plans[(k, 11)]) for k in (29, 30, 38)] == [3, 4, 4]
    # past the four passes the header returns an empty plan (the native program checked npass == 0 and its canaries) and
    # the restatement raises
    refused = {tuple(map(int, ln.split()[1:])) for ln in REFUSED_LINES}
    assert {(k, 11) for k in range(39, 65)} | {(k, 8) for k in range(27, 65)} | {(-1, 11), (5, 2)} == refused
    with pytest.raises(ValueError):
        ns.plan(39, 11)
    with pytest.raises(ValueError):
        ns.plan(27, 8)


@pytest.mark.parametrize("k", range(8, 17))
def test_tiles_partition_the_vector_and_hold_every_butterfly(k):
    """ntt_pass_kernel's (blockIdx.x, slot) -> global index map for every pass of the plan at 2^k: each index of [0, n)
    is held by exactly one slot of one tile, and a tile holds, with any index, the partner that differs in one bit of
    s0 .. s1-1 -- so every butterfly of stages s0+1 .. s1 finds both operands in its own tile's LDS."""
    tb = ns.tile_bits(k)
    n = 1 << k
    for s0, s1, cbits in ns.plan(k, tb):
        gi = ns.tile_indices(k, tb, s0, s1, cbits)
        assert gi.shape == (n >> tb, 1 << tb)
        assert gi.min() == 0 and gi.max() == n - 1
        assert np.array_equal(np.sort(gi.reshape(-1)), np.arange(n)), (k, s0, s1)
        owner = np.empty(n, dtype=np.int64)
        owner[gi.reshape(-1)] = np.repeat(np.arange(gi.shape[0]), gi.shape[1])
        idx = np.arange(n)
        for b in range(s0, s1):
            assert np.array_equal(owner[idx ^ (1 << b)], owner), (k, s0, s1, b)
        # ... and a tile varies exactly tb index bits: its columns, its rows, and whole [r][c] blocks above them
        hbbits = tb - (s1 - s0) - cbits
        free = set(range(cbits)) | set(range(s0, s1)) | set(range(s1, s1 + hbbits))
        assert len(free) == tb
        for b in range(k):
            assert np.array_equal(owner[idx ^ (1 << b)], owner) == (b in free), (k, s0, s1, b)


def test_grids_name_every_size_the_issue_lists():
    """The parametrisation of tests/test_gpu_ntt_sizes.py comes from ntt_sizes: every log_n from 0 to 24 for fft1 (BN254
    l = 2; 0..20 for the other l and curves), 25..27 sampled, and every shape of the pass kernel occurs in it."""
    full = set(ns.FFT1_FULL)
    assert {("bn254", 2, k) for k in range(25)} <= full
    assert {("bn254", l, k) for l in (1, 4, 8) for k in range(21)} <= full
    assert {(c, 2, k) for c in ("bls12_381", "bls12_377") for k in range(21)} <= full
    assert ns.FFT1_SAMPLED == [("bn254", 2, 25), ("bn254", 2, 26), ("bn254", 2, 27)]
    shapes = set()
    for _c, _l, k in ns.FFT1_FULL + ns.FFT1_SAMPLED:
        tb = ns.tile_bits(k)
        if tb is None:
            continue
        for i, (s0, s1, cb) in enumerate(ns.plan(k, tb)):
            sh = ns.pass_shape(k, tb, s0, s1, cb)
            shapes.add((tb, i > 0, sh["odd"], sh["rows"], sh["tws"]))
    # both tiles x first / later pass x odd / even prologue; later passes of the small tile with and without whole rows
    for tb in (8, 11):
        for later in (False, True):
            for odd in (0, 1):
                assert any(s[:3] == (tb, later, odd) for s in shapes), (tb, later, odd)
    # tile origin: a first pass always takes the whole-row branch (with hbbits > 0 and, at full tiles, with hbbits == 0
    # and cbits == s0 == 0); a later pass of a reachable plan always takes the column branch (s1 > tb there)
    assert all(s[3] != s[1] for s in shapes)
    hb = {ns.pass_shape(k, ns.tile_bits(k), *ns.plan(k)[0])["hb"] for _c, _l, k in ns.FFT1_FULL if k >= 8}
    assert hb == {False, True}
    assert {s[4] for s in shapes} == {0, 2}
    # the largest LDS twiddle table: pass 0 of 2^20 takes all 11 stages of the large tile
    assert ns.plan(20)[0] == (0, 11, 0)
    assert all(ns.plan(k)[0][1] < 11 for k in range(15, 28) if k != 20)
