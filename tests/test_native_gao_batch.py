"""The shared text of zk_pss_repair_batch in csrc/gao.hpp is host + device code: gao_batch_entry packs (item, chunk) into the
32-bit entry of the one dirty list as item * nchunks + chunk, gao_batch_decode takes it apart again, gao_batch_fits is the
refusal for nitems * nchunks >= 2^32 (and nitems outside 1 .. 48), gao_layout (without tables) lays out the working
memory.  They are compiled for the host (tests/native/gao_batch_host_test.cpp) and checked against Python integers for
nitems in 1 .. 48 and nchunks in {1, 4, 511, 512, 2^20}, at the first, last and boundary entries of every item.  The same
stand-alone program is built once more with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "zk-saas_amd", "csrc")
_exe = {}
NCHUNKS = [1, 4, 511, 512, 1 << 20]
MAX_ITEMS = 48


def _build(sanitize):
    if sanitize not in _exe:
        out = os.path.join(ROOT, "tests", "native", "_build")
        os.makedirs(out, exist_ok=True)
        exe = os.path.join(out, "gao_batch_host_test" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        r = subprocess.run([CXX, "-std=c++17", "-I" + CSRC] + flags +
                           [os.path.join(ROOT, "tests", "native", "gao_batch_host_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _exe[sanitize] = exe
    return _exe[sanitize]


def _run(sanitize, lines):
    r = subprocess.run([_build(sanitize)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def _entry_cases():
    cases = []
    for nitems in range(1, MAX_ITEMS + 1):
        for nch in NCHUNKS:
            # the first and the last entry of the batch, and both sides of every boundary between two items
            items = sorted({0, 1, nitems // 2, nitems - 2, nitems - 1} & set(range(nitems)))
            for item in items:
                for chunk in sorted({0, 1, nch // 2, nch - 2, nch - 1} & set(range(nch))):
                    cases.append((nitems, nch, item, chunk))
    return cases


def _fits_cases():
    """(nitems, nchunks, fits)"""
    cases = [(0, 4, 0), (49, 4, 0), (48, 4, 1), (1, (1 << 32) - 1, 1), (1, 1 << 32, 0), (2, 1 << 31, 0), (2, (1 << 31) - 1, 1),
             (3, 1431655765, 1), (3, 1431655766, 0), (48, 89478485, 1), (48, 89478486, 0), (7, 1 << 40, 0), (1, 0, 1),
             (48, 1 << 63, 0)]
    for nitems in range(1, MAX_ITEMS + 1):
        edge = -(-(1 << 32) // nitems)                   # the smallest nchunks with nitems * nchunks >= 2^32
        cases += [(nitems, edge - 1, 1), (nitems, edge, 0)] + [(nitems, nch, 1) for nch in NCHUNKS]
    for nitems, nch, want in cases:
        assert want == int(1 <= nitems <= MAX_ITEMS and nch < 1 << 32 and nitems * nch < 1 << 32)
    return cases


def _check(sanitize):
    cases = _entry_cases()
    rows = _run(sanitize, ["e %d %d %d %d" % c for c in cases])
    seen = {}
    for (nitems, nch, item, chunk), row in zip(cases, rows):
        assert row == [item * nch + chunk, item, chunk], (nitems, nch, item, chunk)
        assert row[0] < 1 << 32
        # one entry names one chunk of one item
        assert seen.setdefault((nch, row[0]), (item, chunk)) == (item, chunk)
    fits = _fits_cases()
    assert [r[0] for r in _run(sanitize, ["f %d %d" % c[:2] for c in fits])] == [c[2] for c in fits]
    work = [(n, nitems, nch) for n in (4, 8, 16, 32) for nitems in (1, 3, 7, 48) for nch in NCHUNKS]
    for (n, nitems, nch), (head, total) in zip(work, _run(sanitize, ["w %d %d %d" % c for c in work])):
        assert head % 32 == 0 and head >= 32 + nitems * (3 + n) * 8 and head - 32 < 32 + nitems * (3 + n) * 8
        assert total == head + 4 * nitems * nch


def test_host_entry_packing_decode_and_refusal():
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(False)


def test_host_entry_packing_under_asan_ubsan():
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(True)
