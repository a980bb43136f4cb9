"""tests/gao_model.py, the Python statement of the error-correcting unpack: pinned to the two known answers the reference
holds (tests/golden/gao_f17.json), to oracle.pss unpack / unpack2 on clean words, to an exhaustive search over a small field,
and to the guarantee "at most cap errors => the original message and the exact positions" for every packing factor."""
import json
import os
import random

import pytest

import gao_model as gm
from oracle.params import BLS12_377, BLS12_381, BN254
from oracle.pss import PackedSharingParams as OPP

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gao_f17.json")))


def _f17_root(n):
    """the generator of the size-n subgroup as ark_ff derives it for F17 with generator 3: 3^(16 / n)"""
    return pow(3, 16 // n, 17)


def test_partial_xgcd_known_answer():
    t = GOLD["partial_xgcd"]
    r, s = gm.partial_xgcd(t["a"], t["b"], t["codelength"], t["dimension"], GOLD["modulus"])
    assert r == t["r"] and s == t["s"]


def test_error_correction_known_answer():
    t, p = GOLD["error_correction"], GOLD["modulus"]
    w = _f17_root(t["n"])
    code = gm.encode(t["message"], t["n"], w, p)
    code[t["error_position"]] = (code[t["error_position"]] + t["error_value"]) % p
    got = gm.decode(code, t["k"], w, p)
    assert got.status == 1 and got.errpos == 1 << t["error_position"]
    assert gm.trim(got.message) == t["decoded"]


def test_exhaustive_agreement_over_f17():
    """n = 8, k = 4 (cap 2) and k = 6 (cap 1) over F17: status 1 exactly when the search finds a codeword within cap, and then
    it is the one the search finds (uniqueness: two such codewords would be within 2 cap < n - k + 1 of each other)"""
    p, n = 17, 8
    w = _f17_root(n)
    rnd = random.Random(5)
    for k in (4, 6):
        cap = (n - k) // 2
        for trial in range(120):
            msg = [rnd.randrange(p) for _ in range(k)]
            y = gm.encode(msg, n, w, p)
            for i in rnd.sample(range(n), rnd.randrange(0, cap + 3)):
                y[i] = (y[i] + rnd.randrange(1, p)) % p
            got = gm.decode(y, k, w, p)
            near = gm.brute_force(y, k, w, p)
            assert len(near) <= 1
            if near:
                assert got.status in (0, 1) and tuple(got.message) in near
                code = gm.encode(got.message, n, w, p)
                assert got.errpos == sum(1 << i for i in range(n) if code[i] != y[i])
                assert (got.status == 0) == (got.errpos == 0)
            else:
                assert got == gm.Decoded(2, [0] * k, 0)


@pytest.mark.parametrize("l", [1, 2, 4, 8])
@pytest.mark.parametrize("curve", [BN254, BLS12_381, BLS12_377], ids=["bn254", "bls12_381", "bls12_377"])
def test_clean_words_equal_the_oracle_unpack(curve, l):
    o = OPP(curve, l)
    p, n, w = o.p, o.n, o.share.group_gen
    rnd = random.Random(l)
    sec = [rnd.randrange(p) for _ in range(l)]
    shares = o.pack(sec, [rnd.randrange(p) for _ in range(l)])
    got = gm.decode(shares, 2 * l, w, p)
    assert got.status == 0 and got.errpos == 0
    w2l = o.secret.group_gen
    assert gm.secrets(got.message, l, curve.r_gen, w2l, p) == o.unpack(shares) == sec
    # product shares: degree <= 4l - 2, dimension 4l - 1, secrets at the even points of unpack2's domain
    other = o.pack([rnd.randrange(p) for _ in range(l)], [rnd.randrange(p) for _ in range(l)])
    prod = [a * b % p for a, b in zip(shares, other)]
    got2 = gm.decode(prod, n - 1, w, p)
    assert got2.status == 0
    assert gm.secrets(got2.message, l, curve.r_gen, w2l, p) == o.unpack2(prod)


@pytest.mark.parametrize("l", [1, 2, 4, 8])
def test_up_to_cap_errors_are_corrected_exactly(l):
    curve = BN254
    o = OPP(curve, l)
    p, n, w = o.p, o.n, o.share.group_gen
    rnd = random.Random(100 + l)
    for k in sorted({2 * l, 3 * l, 4 * l - 1}):
        cap = (n - k) // 2
        for e in range(0, cap + 1):
            for trial in range(3):
                msg = [rnd.randrange(p) for _ in range(k)]
                y = gm.encode(msg, n, w, p)
                pos = rnd.sample(range(n), e)
                for i in pos:
                    y[i] = (y[i] + rnd.randrange(1, p)) % p
                got = gm.decode(y, k, w, p)
                assert got == gm.Decoded(1 if e else 0, msg, sum(1 << i for i in pos)), (l, k, e)
        # one error past the capacity of the product code is detected
        if k == n - 1:
            y = gm.encode([rnd.randrange(p) for _ in range(k)], n, w, p)
            y[rnd.randrange(n)] += 1
            assert gm.decode(y, k, w, p).status == 2


def test_case_list_covers_every_class():
    o = OPP(BN254, 2)
    cases = gm.case_list(2, o.p, o.share.group_gen, 1)
    names = " ".join(c[0] for c in cases)
    for word in ("first", "last", "tozero", "zeromsg", "topzero", "second_codeword", "capplus1", "k1_", "k7_", "k4_", "k6_"):
        assert word in names, word
    st = {gm.decode(y, k, o.share.group_gen, o.p).status for _, k, y in cases}
    assert st == {0, 1, 2}
    # the top coefficient of the interpolant vanishes in the "topzero" cases
    for name, k, y in cases:
        if name.endswith("topzero"):
            assert len(gm.interpolate(y, o.share.group_gen, o.p)) < o.n
        if name.endswith("second_codeword"):
            assert gm.decode(y, k, o.share.group_gen, o.p).status == 1
