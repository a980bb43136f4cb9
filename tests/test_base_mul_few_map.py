"""zk_base_mul_few gives a scalar to a group of 8 lanes; csrc/base_mul_few_map.hpp says which windows a lane takes, where
their digits sit in the canonical limbs and who adds whose partial sum at each level of the tree.  Checked on the CPU
(tests/native/base_mul_few_map_host_test.cpp): every window below nwin is taken exactly once for nwin = 1..32, the
digits equal plain byte indexing of random scalars, and lane 0 ends the tree with all eight sums, each once.  The window
map is restated here in Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


def test_lane_group_map_covers_every_window_once_and_the_tree_sums_every_lane():
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found")
    out = os.path.join(ROOT, "tests", "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "base_mul_few_map_host_test")
    r = subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "zk-saas_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "base_mul_few_map_host_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 violations", r.stdout[-4000:]
    windows = sum(range(1, 33))                       # nwin windows for every nwin in 1..32
    digits = 4 * 200 * 8 * 4                          # limb counts x scalars x lanes x digits per lane
    assert lines[-2] == "windows %d digits %d" % (windows, digits)


def test_the_map_is_window_equals_lane_plus_eight_k():
    lanes, per = 8, 4
    taken = sorted(g + lanes * k for g in range(lanes) for k in range(per))
    assert taken == list(range(32))
    for g in range(lanes):
        for k in range(per):
            w = g + lanes * k
            assert (w // 4, 8 * (w % 4)) == (2 * k + (g >> 2), 8 * (g & 3))
