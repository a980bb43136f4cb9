"""csrc/setup.hpp is host + device code: the per-element functions of the quotient kernel of zk_groth16_setup_scalars (the
Lagrange coefficients at tau, h_query in closed form) and the batch inversion a lane runs over its run of indices are
compiled for the host (tests/native/setup_host_test.cpp) and compared with oracle.groth16 on BN254 and BLS12-381 for
m = 2, 8 and 64, with run lengths that divide m and run lengths that leave a short last run."""
import os
import re
import subprocess

import pytest

from oracle import groth16 as og
from oracle.field import Domain, inv_mod
from oracle.params import BLS12_381, BN254

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "zk-saas_amd", "csrc")
_exe = {}


def _build():
    if "exe" not in _exe:
        out = os.path.join(ROOT, "tests", "native", "_build")
        os.makedirs(out, exist_ok=True)
        exe = os.path.join(out, "setup_host_test")
        r = subprocess.run([CXX, "-O2", "-std=c++17", "-I" + CSRC, os.path.join(ROOT, "tests", "native", "setup_host_test.cpp"),
                            "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _exe["exe"] = exe
    return _exe["exe"]


def _run(curve_name, which, m, run, consts):
    r = subprocess.run([_build(), curve_name, which, str(m), str(run)] + ["%x" % c for c in consts], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr
    vals = [int(ln, 16) for ln in r.stdout.split()]
    assert len(vals) == m
    return vals


def _trivial_r1cs(m):
    """nc + ni = m exactly: the Lagrange coefficients and h_query depend on the domain and the trapdoor only"""
    nc = m - 1
    return og.R1CS(1, 1, [[(1, 0)]] * nc, [[(1, 1)]] * nc, [[(1, 1)]] * nc)


# run lengths: 1, divisors of m, the full vector, longer than the vector, and lengths that leave a short last run
RUNS = {2: [1, 2, 3, 16], 8: [1, 2, 3, 4, 5, 7, 8, 16], 64: [1, 3, 7, 16, 32, 48, 63, 64, 65]}


@pytest.mark.parametrize("m", [2, 8, 64])
@pytest.mark.parametrize("curve,name", [(BN254, "bn254"), (BLS12_381, "bls381")], ids=["bn254", "bls12_381"])
def test_quotient_runs_equal_the_oracle(curve, name, m):
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found (field.hpp uses clang's __builtin_addc / __builtin_subc)")
    p = curve.r
    r1 = _trivial_r1cs(m)
    td = og.Trapdoor.from_seed(1000 + m, p)
    key = og.setup_scalars(curve, r1, td)
    assert key.domain.size == m
    dom, dom2 = Domain(curve, m), Domain(curve, 2 * m)
    want_u = og.lagrange_coeffs_at(dom, td.tau)
    w, w2 = dom.group_gen, dom2.group_gen
    assert w2 * w2 % p == w
    lag = [td.tau, (pow(td.tau, m, p) - 1) * inv_mod(m, p) % p, w, inv_mod(w, p)]
    w2i = inv_mod(w2, p)
    h = [td.tau, pow(td.tau, 2 * m, p), inv_mod(td.delta * 2 * m % p, p), w2i * w2i % p, w, w2i]
    for run in RUNS[m]:
        assert _run(name, "lagrange", m, run, lag) == want_u, (m, run)
        assert _run(name, "h", m, run, h) == key.h_query, (m, run)


def test_wrapper_constants_mirror_the_kernel_header():
    """groth16.SETUP_HEAVY_MIN (read by the GPU test of the long-column path) is the constant the kernels are built with"""
    src = open(os.path.join(CSRC, "setup_impl.hpp")).read()
    val = int(re.search(r"constexpr uint32_t SETUP_HEAVY_MIN = (\d+);", src).group(1))
    text = open(os.path.join(ROOT, "zk-saas_amd", "groth16.py")).read()
    assert int(re.search(r"^SETUP_HEAVY_MIN = (\d+)", text, re.M).group(1)) == val
