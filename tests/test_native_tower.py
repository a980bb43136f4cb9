"""csrc/tower.hpp's single-lane Fq6 / Fq12 tower, compiled for the host (tests/native/tower_host_test.cpp) and compared
with oracle.pairing.Tower on BN254 and BLS12-381: mul, sqr, inverse, conjugate, Frobenius 1..3 and the sparse line
product on 24 random values and on values whose coefficients are 0, 1 and q - 1; the cyclotomic squaring against `sqr` on
values already raised to (q^6 - 1)(q^2 + 1).  Integers: every comparison is exact."""
import functools
import os
import random
import subprocess

import pytest

from oracle.pairing import pairing_for
from oracle.params import BLS12_381, BN254

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NRANDOM = 24


def flat(f):
    return [a for h in f for b in h for a in b]


def unflat(v):
    return tuple(tuple((v[6 * h + 2 * b], v[6 * h + 2 * b + 1]) for b in range(3)) for h in range(2))


def line_element(T, twist, l0, ls, l3):
    z = T.zero2
    # l0 + ls w + l3 w^3 (D) or l0 + ls w^2 + l3 w^3 (M); w^j sits in c_{j mod 2}.b_{j div 2}
    return ((l0, z, z), (ls, l3, z)) if twist == "D" else ((l0, ls, z), (z, l3, z))


@functools.lru_cache(maxsize=None)
def frob_coeff(name, j, k):
    pr = pairing_for(BN254 if name == "bn254" else BLS12_381)
    return pr.T.pow2(pr.T.xi, j * (pr.q ** k - 1) // 6)


def frob_ref(pr, a, k):
    """a^(q^k) from the oracle Tower's Fq2 operations: conj^k of the coefficient of w^j (c_{j mod 2}.b_{j div 2}) times
    XI^(j (q^k - 1) / 6).  A power by q^k through pow12 is ~0.1 s of Python, so cases() checks this form against pow12 once
    per k and curve and uses it for every value."""
    T = pr.T
    out = [[None] * 3, [None] * 3]
    for j in range(6):
        x = a[j % 2][j // 2]
        out[j % 2][j // 2] = T.mul2(T.conj2(x) if k & 1 else x, frob_coeff(pr.curve.name, j, k))
    return (tuple(out[0]), tuple(out[1]))


def cases(curve):
    pr = pairing_for(curve)
    T, q = pr.T, curve.q
    rnd = random.Random(0x70 + len(curve.name))
    rand12 = lambda: unflat([rnd.randrange(q) for _ in range(12)])
    vals = [rand12() for _ in range(NRANDOM)]
    for k in (1, 2, 3):
        assert frob_ref(pr, vals[0], k) == T.pow12(vals[0], q ** k)
    vals += [unflat([c] * 12) for c in (1, q - 1)] + [unflat([q - 1, 0, 1] * 4), unflat([0] * 11 + [1]), T.one12]
    out = []
    for i, a in enumerate(vals):
        b = vals[(i * 7 + 3) % len(vals)]
        out.append(("mul", a, b, T.mul12(a, b)))
        out.append(("sqr", a, b, T.mul12(a, a)))
        out.append(("inv", a, b, T.inv12(a)))
        out.append(("conj", a, b, T.conj12(a)))
        for k in (1, 2, 3):
            out.append(("frob%d" % k, a, b, frob_ref(pr, a, k)))
        l = flat(b)[:6]
        out.append(("line", a, b, T.mul12(a, line_element(T, pr.twist, (l[0], l[1]), (l[2], l[3]), (l[4], l[5])))))
    zero = unflat([0] * 12)
    out.append(("mul", zero, vals[0], zero))
    out.append(("sqr", zero, zero, zero))
    for a in vals[:8]:                       # into the cyclotomic subgroup: a^((q^6 - 1)(q^2 + 1))
        e = T.mul12(T.conj12(a), T.inv12(a))
        c = T.mul12(T.pow12(e, q * q), e)
        out.append(("cyc", c, c, T.mul12(c, c)))
    return out


def test_single_lane_tower_equals_the_oracle_tower():
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    out = os.path.join(ROOT, "tests", "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "tower_host_test")
    r = subprocess.run([CXX, "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "zk-saas_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "tower_host_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    todo = [(c.name,) + k for c in (BN254, BLS12_381) for k in cases(c)]
    text = "".join("%s %s %s\n" % (name, op, " ".join("%x" % v for v in flat(a) + flat(b))) for name, op, a, b, _ in todo)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(todo)
    for (name, op, a, b, want), ln in zip(todo, lines):
        assert [int(x, 16) for x in ln.split()] == flat(want), (name, op)
    assert {op for _, op, _, _, _ in todo} == {"mul", "sqr", "inv", "conj", "frob1", "frob2", "frob3", "line", "cyc"}
