"""Reduce stage B of the MSM sums, per bit slice j, the rows (columns) whose index has bit j set; its quads enumerate those
indices with csrc/msm_plan.hpp msm_slice_index / msm_slice_count.  Checked on the CPU for every HI = 2^hb rows + the row
of k = B and every LO = 2^lo_bits columns, hb and lo_bits in 0..10 (tests/native/msm_tail_index_host_test.cpp): exactly
the set with the bit, each index once, increasing, row HI in slice hb only.  The same map is restated here in Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


def test_slice_enumeration_is_the_set_with_the_bit_once_and_in_order():
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found")
    out = os.path.join(ROOT, "tests", "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "msm_tail_index_host_test")
    r = subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "zk-saas_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "msm_tail_index_host_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 violations", r.stdout[-4000:]
    # rows: sum over hb of (hb slices of HI / 2 rows + the top slice of one row); columns: lo_bits slices of LO / 2
    slices = sum(hb + 1 for hb in range(11)) + sum(range(11))
    indices = sum(hb * (1 << hb) // 2 + 1 for hb in range(11)) + sum(lb * (1 << lb) // 2 for lb in range(11))
    assert lines[-2] == "slices %d indices %d" % (slices, indices)


def test_the_map_is_t_with_a_one_inserted_at_bit_j():
    for j in range(11):
        got = [((t >> j) << (j + 1)) | (1 << j) | (t & ((1 << j) - 1)) for t in range(1 << 10)]
        assert got == [i for i in range(1 << 11) if (i >> j) & 1]
