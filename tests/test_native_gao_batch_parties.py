"""The shared text of zk_pss_repair_batch_parties in csrc/gao.hpp is host + device code.  tests/native/
gao_batch_parties_host_test.cpp runs it over GaoHostGroup for a batch of 3 items of ONE party list, through working memory
laid out by gao_layout: the scan whose row of party p is the popcount of the `listed` mask, the one dirty list of
gao_batch_entry(item, chunk) entries, and the repair that decodes an entry, loads through the table in working memory and
writes into the item's compact matrix, adding to the item's summary words chunk by chunk.
  cases      gao_erasure_model.case_list_parties, grouped by (dimension, party list) and dealt round-robin to the 3 items, so
             each item carries a different mix of verdicts; over a field all three statuses and a phantom occur
  yardstick  the single-word party-list text that tests/native/gao_repair_parties_host_test.cpp runs, case by case: status,
             errpos and the listed shares after the repair are equal; an item's summary words are the counts of its own
             verdicts (nothing leaks between items); the pad between two items keeps its value
  layout     gao_layout against Python integers, with the tables' real sizes and with made-up ones
  call       tests/native/gao_call_host_test.cpp, which checks itself: gao_layout against the offsets of the layouts it
             replaced, every refusal of gao_list_check and gao_call_check, lists of length 1, n - 1 and n
Fields: F17 at l = 1, 2, 4 and BN254 Fr at l = 1, 2, 4, 8.  The same stand-alone programs are built once more with
-fsanitize=address,undefined."""
import os
import subprocess

import pytest

import gao_erasure_model as em
from test_native_gao_repair_parties import CSRC, CXX, FIELDS, ROOT, _field

_exe = {}
NITEMS = 3
PAD = 3


def _build(name, sanitize):
    if (name, sanitize) not in _exe:
        out = os.path.join(ROOT, "tests", "native", "_build")
        os.makedirs(out, exist_ok=True)
        exe = os.path.join(out, name + ("_bp_san" if sanitize else "_bp"))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        r = subprocess.run([CXX, "-std=c++17", "-I" + CSRC] + flags +
                           [os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _exe[(name, sanitize)] = exe
    return _exe[(name, sanitize)]


def _run(exe, args, text):
    r = subprocess.run([exe] + args, input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def _round32(v):
    return (v + 31) // 32 * 32


def _layout(n, nitems, nch, tab_size, inv_size):
    head = _round32(32 + nitems * (3 + n) * 8)
    inv = head + _round32(tab_size)
    lst = inv + _round32(inv_size)
    return [head, inv, lst, lst + 4 * nitems * nch]


def _batches(l, p, w):
    """[(k, S, items)]: items[i] is the list of (name, word) of item i, all of one length"""
    groups = {}
    for name, k, S, word in em.case_list_parties(l, p, w, 13):
        if len(S) < 4 * l:                       # (all n parties is zk_pss_repair_batch)
            groups.setdefault((k, tuple(S)), []).append((name, word))
    out = []
    for (k, S), cases in groups.items():
        items = [cases[i::NITEMS] for i in range(NITEMS)]
        nch = max(len(it) for it in items)
        for i, it in enumerate(items):
            it += [cases[(i + j) % len(cases)] for j in range(nch - len(it))]
        out.append((k, list(S), items))
    return out


def _check(name, l, sanitize):
    p, w = _field(name, l)
    n = 4 * l
    batches = _batches(l, p, w)
    assert batches
    text, single = [], []
    for k, S, items in batches:
        nch = len(items[0])
        text.append("%d %d %s %d %d %d" % (k, len(S), " ".join(map(str, S)), NITEMS, nch, PAD))
        for it in items:
            for _, word in it:
                text.append(" ".join("%x" % v for v in word))
                single.append("%d %d %s %s" % (k, len(S), " ".join(map(str, S)), " ".join("%x" % v for v in word)))
    got = _run(_build("gao_batch_parties_host_test", sanitize), [name, str(l)], "".join(t + "\n" for t in text))
    want = _run(_build("gao_repair_parties_host_test", sanitize), [name, str(l)], "".join(t + "\n" for t in single))
    gi = wi = 0
    seen, phantom, mixes_differ = set(), False, False
    for k, S, items in batches:
        nch = len(items[0])
        hist, seqs = [], []
        for it in items:
            sums = [0] * (3 + n)
            seqs.append([])
            for cname, word in it:
                assert got[gi] == want[wi], (name, l, k, S, cname)
                st, ep = int(got[gi][0]), int(got[gi][1], 16)
                sums[st] += 1
                for q in range(n):
                    sums[3 + q] += (ep >> q) & 1
                assert not ep & ~sum(1 << q for q in S)
                seen.add(st)
                seqs[-1].append(st)
                if cname.endswith("phantom"):
                    assert st == 2 and [int(v, 16) for v in got[gi][2:]] == list(word)
                    phantom = True
                gi, wi = gi + 1, wi + 1
            hist.append(sums)
        for sums in hist:                          # the item's summary words: its own verdicts, nothing from the others
            assert [int(v) for v in got[gi]] == sums and sum(sums[:3]) == nch, (name, l, k, S)
            gi += 1
        # (the items of a batch differ in where their clean, corrected and failed chunks lie, and in one batch at least
        # every item holds two kinds of verdict)
        mixes_differ = mixes_differ or (len({tuple(q) for q in seqs}) == NITEMS and all(len(set(q)) >= 2 for q in seqs))
        tail = [int(v) for v in got[gi]]
        gi += 1
        assert tail[:4] == _layout(n, NITEMS, nch, tail[4], tail[5]) and tail[6] == 1, (name, l, k, S)
        fb = 8 if name == "f17" else 32            # the tables hold at least their members
        assert tail[4] >= (3 * 32 + 16) * fb + 32 * 4 + 12 and tail[5] == 32 * fb
    assert gi == len(got) and wi == len(want)
    assert seen == {0, 1, 2} and phantom and mixes_differ


def _check_layout(sanitize):
    cases = [(n, nitems, nch, tab, inv) for n in (4, 8, 16, 32) for nitems in (1, 3, 7, 48) for nch in (1, 4, 511, 512, 1 << 20)
             for tab, inv in ((1, 1), (32, 64), (3372, 1024), (4093, 33))]
    rows = _run(_build("gao_batch_parties_host_test", sanitize), ["layout"], "".join("%d %d %d %d %d\n" % c for c in cases))
    assert len(rows) == len(cases)
    for c, row in zip(cases, rows):
        assert [int(v) for v in row] == _layout(*c), c
        assert all(int(v) % 32 == 0 for v in row[:3])


def _need_cxx():
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")


@pytest.mark.parametrize("name,l", FIELDS, ids=["%s_l%d" % f for f in FIELDS])
def test_host_batch_parties_equals_the_single_word_text(name, l):
    _need_cxx()
    _check(name, l, False)


@pytest.mark.parametrize("name,l", FIELDS, ids=["%s_l%d" % f for f in FIELDS])
def test_host_batch_parties_under_asan_ubsan(name, l):
    _need_cxx()
    _check(name, l, True)


def test_host_working_memory_layout():
    _need_cxx()
    _check_layout(False)


def test_host_working_memory_layout_under_asan_ubsan():
    _need_cxx()
    _check_layout(True)


def _check_call(sanitize):
    rows = _run(_build("gao_call_host_test", sanitize), [], "")
    assert rows == [["0", "failed"]], rows


def test_host_call_layout_and_refusals():
    _need_cxx()
    _check_call(False)


def test_host_call_layout_and_refusals_under_asan_ubsan():
    _need_cxx()
    _check_call(True)


def _check_call(sanitize):
    rows = _run(_build("gao_call_host_test", sanitize), [], "")
    assert rows == [["0", "failed"]], rows


def test_host_call_layout_and_refusals():
    _need_cxx()
    _check_call(False)


def test_host_call_layout_and_refusals_under_asan_ubsan():
    _need_cxx()
    _check_call(True)
