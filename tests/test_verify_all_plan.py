"""The host-only part of zk_groth16_verify_all (csrc/pairing_rlc_plan.hpp), checked on the CPU through
tests/native/rlc_host_test.cpp: the derivation of the randomizers from the seed against a ChaCha20 written here (pinned on
the RFC 7539 section 2.3.2 vector), and the split of the Miller values' product over lane groups for every n in 1..5000."""
import functools
import math
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NONCE = 0x5A4B524C43
M32 = 0xFFFFFFFF


def chacha20_block(key_words, counter, nonce):
    """RFC 7539 2.3 with words 12, 13 = the 64-bit counter and 14, 15 = the 64-bit nonce (little endian halves)"""
    s = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(key_words) + [counter & M32, counter >> 32, nonce & M32, nonce >> 32]
    x = list(s)
    rot = lambda v, n: ((v << n) | (v >> (32 - n))) & M32

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & M32; x[d] = rot(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & M32; x[b] = rot(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & M32; x[d] = rot(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & M32; x[b] = rot(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(x, s)]


def randomizer(seed, i):
    """what the header documents: r_i = w0 | w1 << 32 | w2 << 64 | w3 << 96, a zero draw replaced by 1"""
    w = chacha20_block(struct.unpack("<8I", seed), i, NONCE)
    return (w[0] | w[1] << 32 | w[2] << 64 | w[3] << 96) or 1


@functools.lru_cache(maxsize=None)
def _exe():
    if not os.path.exists(CXX):
        pytest.skip("ROCm host compiler not found")
    out = os.path.join(ROOT, "tests", "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "rlc_host_test")
    r = subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-variable", "-Wno-unused-function",
                        "-I" + os.path.join(ROOT, "zk-saas_amd", "csrc"), os.path.join(ROOT, "tests", "native", "rlc_host_test.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(*args):
    r = subprocess.run([_exe(), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    return r.stdout.splitlines()


def test_the_chacha20_written_here_gives_the_rfc_7539_vector():
    w = chacha20_block(struct.unpack("<8I", bytes(range(32))), 1 | (0x09000000 << 32), 0x4A000000)
    assert struct.pack("<16I", *w).hex() == (
        "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
        "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")


SEEDS = [bytes(32), b"\xff" * 32, bytes.fromhex("8f1d3a5c7e9b0d2f4a6c8e0b1d3f5a7c9e0b2d4f6a8c0e1f3b5d7f9a1c3e5f70")]
INDICES = [0, 1, 1 << 32, (1 << 32) + 1]


@pytest.mark.parametrize("seed", SEEDS, ids=["zero", "ff", "random"])
def test_randomizers_are_the_first_four_words_of_the_block_little_endian(seed):
    lines = _run("rand", seed.hex(), *map(str, INDICES))
    assert len(lines) == len(INDICES)
    got = {}
    for ln in lines:
        tag, idx, *words = ln.split()
        assert tag == "r" and len(words) == 4
        got[int(idx)] = sum(int(w, 16) << (32 * j) for j, w in enumerate(words))
    assert got == {i: randomizer(seed, i) for i in INDICES}
    assert len(set(got.values())) == len(INDICES) and all(0 < v < 1 << 128 for v in got.values())
    # the counter is 64 bits wide: index 2^32 is not index 0 again, and the high word sits in word 13
    assert chacha20_block(struct.unpack("<8I", seed), 1 << 32, NONCE) != chacha20_block(struct.unpack("<8I", seed), 0, NONCE)


def test_a_zero_draw_becomes_one():
    assert _run("zero") == ["zero ok"]


def test_gt_fold_plan_for_every_n_up_to_5000():
    lines = _run("plan", "5000")
    assert lines[-1] == "0 violations", "\n".join(lines[-45:])
    rows = [tuple(map(int, ln.split()[1:])) for ln in lines if ln.startswith("plan ")]
    assert [r[0] for r in rows] == list(range(1, 5001))
    for n, G, ln, empties in rows:
        bound = math.isqrt(n - 1) + 2                    # ceil(sqrt(n)) + 1
        assert 1 <= G <= bound and 1 <= ln <= bound, (n, G, ln)
        assert (G - empties - 1) * ln < n <= (G - empties) * ln, (n, G, ln, empties)      # the non-empty groups cover 0..n-1
    # the sizes the GPU test sits on: count + 3 = 8, 9, 32, 33, 64, 65, 303
    plan = {r[0]: r[1:] for r in rows}
    assert [plan[n][:2] for n in (4, 5, 8, 9, 32, 33, 64, 65, 303)] == [(2, 2), (3, 2), (3, 3), (3, 3), (6, 6), (6, 6), (8, 8),
                                                                        (9, 8), (18, 17)]
