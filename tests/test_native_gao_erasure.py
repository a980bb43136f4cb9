"""The absent-party forms of csrc/gao.hpp (zk_pss_unpack_robust_parties) are host + device code: the table of a party list,
stage 1's multiplying load, clean test, secrets and root-by-root deflation, and stage 2's decoder with gao_absent_finish are
compiled for the host (tests/native/gao_erasure_host_test.cpp) and compared with tests/gao_erasure_model.py case for case --
status, message, errpos and secrets -- for l = 1, 2, 4, 8 on BN254 and BLS12-381, over gao_erasure_model.case_list_parties.
The same program is built once more with -fsanitize=address,undefined and run directly."""
import os
import subprocess

import pytest

import gao_erasure_model as em
import gao_model as gm
from oracle.params import BLS12_381, BN254
from oracle.pss import PackedSharingParams as OPP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "zk-saas_amd", "csrc")
_exe = {}
CURVES = [(BN254, "bn254"), (BLS12_381, "bls381")]


def _build(sanitize):
    if sanitize not in _exe:
        out = os.path.join(ROOT, "tests", "native", "_build")
        os.makedirs(out, exist_ok=True)
        exe = os.path.join(out, "gao_erasure_host_test" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        r = subprocess.run([CXX, "-std=c++17", "-I" + CSRC] + flags +
                           [os.path.join(ROOT, "tests", "native", "gao_erasure_host_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _exe[sanitize] = exe
    return _exe[sanitize]


def _run(exe, name, l, cases):
    text = "".join("%d %d %s %s\n" % (k, len(S), " ".join(map(str, S)), " ".join("%x" % v for v in word))
                   for _, k, S, word in cases)
    r = subprocess.run([exe, name, str(l)], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def _check(curve, name, l, sanitize):
    o = OPP(curve, l)
    p, w = o.p, o.share.group_gen
    cases = em.case_list_parties(l, p, w, 7)
    rows = _run(_build(sanitize), name, l, cases)
    seen, demoted = set(), 0
    for (cname, k, S, word), row in zip(cases, rows):
        want = em.decode(word, S, k, w, p)
        sec = gm.secrets(want.message, l, curve.r_gen, o.secret.group_gen, p) if want.status != 2 else [0] * l
        got_status, got_err = int(row[0]), int(row[1], 16)
        got_msg = [int(v, 16) for v in row[2:2 + k]]
        got_sec = [int(v, 16) for v in row[2 + k:]]
        assert (got_status, got_msg, got_err, got_sec) == (want.status, want.message, want.errpos, sec), (name, l, cname)
        seen.add(want.status)
        demoted += "phantom" in cname
    assert seen == {0, 1, 2} and demoted


@pytest.mark.parametrize("l", [1, 2, 4, 8])
@pytest.mark.parametrize("curve,name", CURVES, ids=[c[1] for c in CURVES])
def test_host_absent_forms_equal_the_model(curve, name, l):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(curve, name, l, False)


@pytest.mark.parametrize("l", [1, 2, 4, 8])
def test_host_absent_forms_under_asan_ubsan(l):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(BN254, "bn254", l, True)
