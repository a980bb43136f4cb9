"""The chunk ranges of the all-to-all king and the column -> chunk map that the range form of the repair writes its verdicts
through are one host + device text, csrc/king_range.hpp (king_span, king_chunk, GaoRange): engine_dist.inc.hpp a2a_plan cuts
the ranges with it and gao_impl.hpp's range kernels index status and errpos with it.  tests/native/king_range_host_test.cpp
runs it on the CPU for every (len, present ranks, granule, shift) with len in {8 .. 8192, powers of two}, 2 .. 8 ranks,
granule 1 and 256 (capped at len), shift 0 and 1:
  * the ranges of all present ranks hit every chunk 0 .. len - 1 exactly once,
  * no column >= cnt is mapped, and the columns below cnt are the ones the pack kernel fills,
  * the plan applies exactly when there is a granule per rank.
Built and run once plain and once with -fsanitize=address,undefined.  The case counts are restated here in Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


def _expected():
    cases = applicable = chunks = 0
    ln = 8
    while ln <= 8192:
        for ranks in range(2, 9):
            for gran in (1, min(ln, 256)):
                for _shift in (0, 1):
                    cases += 1
                    if ln // gran >= ranks:
                        applicable += 1
                        chunks += ln
        ln *= 2
    return cases, applicable, chunks


def _run(sanitize):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found")
    out = os.path.join(ROOT, "tests", "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "king_range_host_test" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    r = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "zk-saas_amd", "csrc")] + flags +
                       [os.path.join(ROOT, "tests", "native", "king_range_host_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 violations", r.stdout[-4000:]
    assert lines[-2] == "cases %d applicable %d chunks %d" % _expected()


def test_ranges_cover_every_chunk_once_and_map_no_padding():
    _run(False)


def test_ranges_under_asan_ubsan():
    _run(True)

