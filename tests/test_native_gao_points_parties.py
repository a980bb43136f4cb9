"""The party-list decoder of csrc/gao_points.hpp (zk_pss_repair_points_parties, zk_pss_unpack_points_robust_parties) is host +
device code: the table of a (list, dimension), the syndrome rows of stage 1 and the lane-group logic of stage 2 are compiled
for the host (tests/native/gao_points_parties_host_test.cpp) over BN254 G1 and compared with
tests/points_robust_parties_model.py at l = 1, 2, 4.  Lists: all present; the first, a middle and the last party absent;
rho = 2l - 2 (the last list that still corrects at k = 2l); rho = 2l - 1 (detection only).  Words: clean, one error at each
listed party, a wrong share that is the identity, two errors; and k = 4l - 1 with all present.  The repaired compact word must
be the lift of the model's repaired scalar word, point for point; the unpack form must give the lift of the model's secrets.
The same stand-alone program is built once more with -fsanitize=address,undefined and run directly."""
import os
import subprocess

import pytest

import gao_model as gm
import points_robust_parties_model as prpm
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
        exe = os.path.join(out, "gao_points_parties_host_test" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        r = subprocess.run([CXX, "-std=c++17", "-I" + CSRC] + flags +
                           [os.path.join(ROOT, "tests", "native", "gao_points_parties_host_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _exe[sanitize] = exe
    return _exe[sanitize]


def _check(l, sanitize):
    o = OPP(BN254, l)
    p, w, n = o.p, o.share.group_gen, 4 * l
    cases = prpm.case_list(l, w, p)
    # (at l = 1 the lists with rho = 2l - 2 and 2l - 1 are among the first four)
    assert {len(S) for _, k, S, _ in cases if k == 2 * l} == {n, n - 1, 2 * l + 2, 2 * l + 1}
    for e in (0, n // 2, n - 1):
        assert any(len(S) == n - 1 and e not in S for _, _, S, _ in cases)
    want = [prpm.repaired(y, S, k, w, p) for _, k, S, y in cases]
    secs = [gm.secrets(d.message, l, o.curve.r_gen, o.secret.group_gen, p) if d.status != 2 else [0] * l for d, _ in want]
    scalars = sorted({v for _, fixed in want for v in fixed} | {v for sec in secs for v in sec})

    def req(tag):
        return "".join("%s %d %d %s %s\n" % (tag, k, len(S), " ".join(map(str, S)), " ".join("%x" % v for v in y))
                       for _, k, S, y in cases)

    text = "".join("L %x\n" % s for s in scalars) + req("W") + req("U")
    r = subprocess.run([_build(sanitize), str(l)], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(scalars) + 2 * len(cases)
    lift = {s: (int(row[0], 16), int(row[1], 16)) for s, row in zip(scalars, rows)}
    G = g1(BN254)
    for s in (scalars[1], scalars[len(scalars) // 2], scalars[-1]):
        assert lift[s] == tuple(G.to_affine(G.mul(G.from_affine(BN254.g1), s)))
    assert lift.get(0, (0, 0)) == (0, 0)
    seen = set()
    for (cname, k, S, y), (d, fixed), row in zip(cases, want, rows[len(scalars):len(scalars) + len(cases)]):
        pts = [(int(row[2 + 2 * i], 16), int(row[3 + 2 * i], 16)) for i in range(len(S))]
        assert (int(row[0]), int(row[1], 16)) == (d.status, d.errpos), (l, cname)
        assert pts == [lift[v] for v in fixed], (l, cname)
        seen.add(d.status)
        assert all((d.errpos >> q) & 1 == 0 for q in range(n) if q not in S)
        if cname.endswith("_clean"):
            assert d.status == 0
        if "_party" in cname:
            q = int(cname.split("party")[1])
            assert (d.status, d.errpos) == ((1, 1 << q) if len(S) - k >= 2 else (2, 0)), (l, cname)
        if "_two_" in cname and len(S) - k >= 4:
            assert d.status == 2, (l, cname)          # minimum distance |S| - k + 1 >= 5: not within one of any codeword
    assert seen == {0, 1, 2}
    for (cname, k, S, y), (d, _), sec, row in zip(cases, want, secs, rows[len(scalars) + len(cases):]):
        assert (int(row[0]), int(row[1], 16)) == (d.status, d.errpos), (l, cname, "unpack")
        pts = [(int(row[2 + 2 * i], 16), int(row[3 + 2 * i], 16)) for i in range(l)]
        assert pts == [lift[v] for v in sec], (l, cname, "unpack")


@pytest.mark.parametrize("l", [1, 2, 4])
def test_host_points_decoder_with_a_party_list_equals_the_model(l):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(l, False)


@pytest.mark.parametrize("l", [1, 2, 4])
def test_host_points_decoder_with_a_party_list_under_asan_ubsan(l):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    _check(l, True)
