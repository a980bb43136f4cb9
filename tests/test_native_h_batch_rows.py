"""The report of a checked batch is proof-major, [nb][7], while the repair of a round indexes its items, so the three repairs
of zk_circom_h_batch_checked write a round-major staging report and one gather launch moves every row to its place.  The row
map is one host + device text, csrc/h_batch.hpp (staging_row, staging_round_first, staging_round_items): the engine places
the repairs with it and h_report_gather_kernel reads through it.  tests/native/h_batch_rows_host_test.cpp runs it on the CPU
for every batch size 1 .. 16:
  * staging_row is a bijection onto 0 .. 7 nb - 1,
  * a round's rows are contiguous and in the item order of its repair,
  * the gather, replayed on host buffers, gives every report row the bytes of its own (proof, item).
and the layout of the chain's work buffer (h_layout, the one place that computes it) for every form of the chain at nb 1 .. 16,
n in {4, 8, 16, 32}, m/l in {1, 4, 512, 2^17}: regions aligned, in order and disjoint, the totals those the four forms asked for
before (written out in the test), no staging for one proof.
Built and run once plain and once with -fsanitize=address,undefined.  The counts are restated here in Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


def _run(sanitize):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found")
    out = os.path.join(ROOT, "tests", "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "h_batch_rows_host_test" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    r = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "zk-saas_amd", "csrc")] + flags +
                       [os.path.join(ROOT, "tests", "native", "h_batch_rows_host_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 violations", r.stdout[-4000:]
    assert lines[-2] == "batches %d rows %d" % (16, sum(7 * nb for nb in range(1, 17)))
    # per field, n and m/l: one proof in 9 forms (unchecked; checked x errpos x summary, with a list and without), a batch in 5
    assert lines[-3] == "layouts %d" % (2 * 4 * 4 * (9 + 15 * 5))


def test_staging_rows_are_a_bijection_and_rounds_are_contiguous():
    _run(False)


def test_staging_rows_under_asan_ubsan():
    _run(True)
