"""The repair form of csrc/gao.hpp with a party list (zk_pss_repair_parties) is host + device code: the scan that loads with
the multiplication by Lambda(w^p), the lane-group decoder with its re-encoding at dimension k + rho, gao_absent_finish on that
result and the store of h'(w^p) / Lambda(w^p) into the party's row are compiled for the host
(tests/native/gao_repair_parties_host_test.cpp) and compared with tests/gao_erasure_model.py case for case over
gao_erasure_model.case_list_parties: status and errpos equal the model's, the listed shares after the repair equal the input
everywhere except at the errpos places of a status-1 case, where they equal poly_eval(message, w^p).  Fields: F17 (gao.rs's
own test field; l <= 4, its largest subgroup has 16 elements) and BN254 Fr at l = 1, 2, 4, 8.  The same stand-alone program
is built once more with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

import gao_erasure_model as em
import gao_model as gm
from oracle.params import BN254
from oracle.pss import PackedSharingParams as OPP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "zk-saas_amd", "csrc")
_exe = {}
FIELDS = [("f17", l) for l in (1, 2, 4)] + [("bn254", l) for l in (1, 2, 4, 8)]


def _build(sanitize):
    if sanitize not in _exe:
        out = os.path.join(ROOT, "tests", "native", "_build")
        os.makedirs(out, exist_ok=True)
        exe = os.path.join(out, "gao_repair_parties_host_test" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        r = subprocess.run([CXX, "-std=c++17", "-I" + CSRC] + flags +
                           [os.path.join(ROOT, "tests", "native", "gao_repair_parties_host_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _exe[sanitize] = exe
    return _exe[sanitize]


def _field(name, l):
    """(p, the generator of the share domain H_4l)"""
    if name == "f17":
        return 17, pow(3, 16 // (4 * l), 17)        # ark_ff's F17 with generator 3
    o = OPP(BN254, l)
    return o.p, o.share.group_gen


def _check(name, l, sanitize):
    p, w = _field(name, l)
    cases = em.case_list_parties(l, p, w, 13)
    text = "".join("%d %d %s %s\n" % (k, len(S), " ".join(map(str, S)), " ".join("%x" % v for v in word))
                   for _, k, S, word in cases)
    r = subprocess.run([_build(sanitize), name, str(l)], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    seen, phantom, absent_seen = set(), False, False
    for (cname, k, S, word), row in zip(cases, rows):
        want = em.decode(word, S, k, w, p)
        fixed = list(word)
        if want.status == 1:
            assert want.errpos and not want.errpos & ~sum(1 << q for q in S)
            for i, q in enumerate(S):
                if (want.errpos >> q) & 1:
                    fixed[i] = gm.poly_eval(want.message, pow(w, q, p), p)
            # (the repaired word is the codeword of the message on the listed points)
            assert fixed == [gm.poly_eval(want.message, pow(w, q, p), p) for q in S]
        got = (int(row[0]), int(row[1], 16), [int(v, 16) for v in row[2:]])
        assert got == (want.status, want.errpos, fixed), (name, l, cname)
        seen.add(want.status)
        absent_seen = absent_seen or (want.status == 1 and len(S) < 4 * l)
        if cname.endswith("phantom"):
            assert want.status == 2 and got[2] == list(word)
            phantom = True
    assert seen == {0, 1, 2} and phantom and absent_seen


@pytest.mark.parametrize("name,l", FIELDS, ids=["%s_l%d" % f for f in FIELDS])
def test_host_repair_parties_equals_the_model(name, l):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(name, l, False)


@pytest.mark.parametrize("name,l", FIELDS, ids=["%s_l%d" % f for f in FIELDS])
def test_host_repair_parties_under_asan_ubsan(name, l):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(name, l, True)
