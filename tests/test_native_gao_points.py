"""The decoder of csrc/gao_points.hpp (zk_pss_repair_points) is host + device code: the syndrome rows of stage 1 and the
lane-group logic of stage 2 are compiled for the host (tests/native/gao_points_host_test.cpp) over BN254 G1 and compared with
tests/points_robust_model.py at l = 1, 2, 4: clean words, one error at each party, two errors, dimension 4l - 1, and
gao_model.case_list.  Status, position and the corrected share are checked against the scalars' truth: the repaired word
must be the lift of the model's repaired scalar word, point for point; the unpack form of the decoder (the secrets of the
corrected word) must give the lift of the model's secrets.  The same stand-alone program is built once more
with -fsanitize=address,undefined and run directly."""
import os
import random
import subprocess

import pytest

import gao_model as gm
import points_robust_model as prm
from oracle.curve import g1
from oracle.params import BN254
from oracle.pss import PackedSharingParams as OPP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "zk-saas_amd", "csrc")
_exe = {}


def _build(sanitize):
    if sanitize not in _exe:
        out = os.path.join(ROOT, "tests", "native", "_build")
        os.makedirs(out, exist_ok=True)
        exe = os.path.join(out, "gao_points_host_test" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        r = subprocess.run([CXX, "-std=c++17", "-I" + CSRC] + flags +
                           [os.path.join(ROOT, "tests", "native", "gao_points_host_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _exe[sanitize] = exe
    return _exe[sanitize]


def _cases(l, p, w):
    """[(name, k, y)]"""
    rnd = random.Random(500 + l)
    n = 4 * l
    cases = []
    for k in (2 * l, 4 * l - 1):
        code = gm.encode([rnd.randrange(1, p) for _ in range(k)], n, w, p)

        def corrupt(pos):
            y = list(code)
            for q in pos:
                y[q] = (y[q] + rnd.randrange(1, p)) % p
            return y

        cases.append(("k%d_clean" % k, k, list(code)))
        cases += [("k%d_party%d" % (k, q), k, corrupt([q])) for q in range(n)]
        cases += [("k%d_two_%d" % (k, t), k, corrupt(rnd.sample(range(n), 2))) for t in range(3)]
        y = list(code)
        y[rnd.randrange(n)] = 0                       # a wrong share that is the identity
        cases.append(("k%d_tozero" % k, k, y))
    cases.append(("zero", 2 * l, [0] * n))
    cases.append(("same", 2 * l, [5] * n))            # a degree-0 codeword: every addition of a row doubles
    return cases + gm.case_list(l, p, w, 7)


def _check(l, sanitize):
    o = OPP(BN254, l)
    p, w, n = o.p, o.share.group_gen, 4 * l
    cases = _cases(l, p, w)
    want = [prm.repaired(y, k, w, p) for _, k, y in cases]
    # the unpack form: the secrets of the decoded message, zeros for a failed word
    secs = [gm.secrets(d.message, l, o.curve.r_gen, o.secret.group_gen, p) if d.status != 2 else [0] * l for d, _ in want]
    scalars = sorted({v for _, fixed in want for v in fixed} | {v for sec in secs for v in sec})
    text = "".join("L %x\n" % s for s in scalars)
    text += "".join("W %d %s\n" % (k, " ".join("%x" % v for v in y)) for _, k, y in cases)
    text += "".join("U %d %s\n" % (k, " ".join("%x" % v for v in y)) for _, k, y in cases)
    r = subprocess.run([_build(sanitize), str(l)], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(scalars) + 2 * len(cases)
    lift = {s: (int(row[0], 16), int(row[1], 16)) for s, row in zip(scalars, rows)}
    # the lift itself, against the oracle's curve arithmetic: three scalars
    G = g1(BN254)
    for s in (scalars[1], scalars[len(scalars) // 2], scalars[-1]):
        assert lift[s] == tuple(G.to_affine(G.mul(G.from_affine(BN254.g1), s)))
    assert lift.get(0, (0, 0)) == (0, 0)
    seen = set()
    for (cname, k, y), (d, fixed), row in zip(cases, want, rows[len(scalars):len(scalars) + len(cases)]):
        pts = [(int(row[2 + 2 * q], 16), int(row[3 + 2 * q], 16)) for q in range(n)]
        assert (int(row[0]), int(row[1], 16)) == (d.status, d.errpos), (l, cname)
        assert pts == [lift[v] for v in fixed], (l, cname)
        seen.add(d.status)
        if cname.endswith("_clean"):
            assert d.status == 0
        if "_party" in cname:
            q = int(cname.split("party")[1])
            assert (d.status, d.errpos) == ((1, 1 << q) if n - k >= 2 else (2, 0)), (l, cname)
        if "_two_" in cname and l >= 2:
            assert d.status == 2, (l, cname)
    assert seen == {0, 1, 2}
    for (cname, k, y), (d, _), sec, row in zip(cases, want, secs, rows[len(scalars) + len(cases):]):
        assert (int(row[0]), int(row[1], 16)) == (d.status, d.errpos), (l, cname, "unpack")
        pts = [(int(row[2 + 2 * i], 16), int(row[3 + 2 * i], 16)) for i in range(l)]
        assert pts == [lift[v] for v in sec], (l, cname, "unpack")


@pytest.mark.parametrize("l", [1, 2, 4])
def test_host_points_decoder_equals_the_model(l):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(l, False)


@pytest.mark.parametrize("l", [1, 2, 4])
def test_host_points_decoder_under_asan_ubsan(l):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(l, True)
