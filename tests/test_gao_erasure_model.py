"""tests/gao_erasure_model.py, the statement of zk_pss_unpack_robust_parties the native and GPU tests compare with, against a
brute-force search over all k-subsets of the listed parties on F17 (n = 4 and 8), against gao_model.decode when every party
is listed, and the coverage its case list promises: all three statuses for every party set that can correct."""
import random

import pytest

import gao_erasure_model as em
import gao_model as gm
from oracle.params import BN254
from oracle.pss import PackedSharingParams as OPP

F17 = [(17, 4, 4), (17, 2, 8)]          # (p, omega, n): omega has order n


@pytest.mark.parametrize("p,omega,n", F17)
def test_model_equals_brute_force(p, omega, n):
    assert pow(omega, n, p) == 1 and pow(omega, n // 2, p) != 1
    rnd = random.Random(n)
    seen = {0: 0, 1: 0, 2: 0}
    for _ in range(1200):
        k = rnd.randrange(1, n)
        m = rnd.randrange(k + 1, n + 1)
        S = sorted(rnd.sample(range(n), m))
        xs = [pow(omega, q, p) for q in S]
        msg = [rnd.randrange(p) for _ in range(k)]
        word = [gm.poly_eval(msg, x, p) for x in xs]
        for i in rnd.sample(range(m), min(m, rnd.randrange(0, (m - k) // 2 + 3))):
            word[i] = (word[i] + rnd.randrange(1, p)) % p
        got = em.decode(word, S, k, omega, p)
        found = em.brute_force(word, S, k, omega, p)
        assert len(found) <= 1, (S, k, word, found)
        if not found:
            assert got == gm.Decoded(2, [0] * k, 0), (S, k, word)
        else:
            (h, err), = found.items()
            assert got == gm.Decoded(1 if err else 0, list(h), err), (S, k, word)
            assert not err & ~sum(1 << q for q in S)
        seen[got.status] += 1
    assert all(seen.values()), seen


@pytest.mark.parametrize("p,omega,n", F17)
def test_all_parties_listed_is_gao_model(p, omega, n):
    rnd = random.Random(100 + n)
    for _ in range(600):
        k = rnd.randrange(1, n)
        y = gm.encode([rnd.randrange(p) for _ in range(k)], n, omega, p)
        for i in rnd.sample(range(n), rnd.randrange(0, (n - k) // 2 + 3)):
            y[i] = (y[i] + rnd.randrange(1, p)) % p
        assert em.decode(y, list(range(n)), k, omega, p) == gm.decode(y, k, omega, p)


@pytest.mark.parametrize("l", [1, 2, 4, 8])
def test_case_list_reaches_every_status_for_every_party_set(l):
    o = OPP(BN254, l)
    p, w, n = o.p, o.share.group_gen, 4 * l
    cases = em.case_list_parties(l, p, w, 7)
    assert cases == em.case_list_parties(l, p, w, 7)
    by_set = {}
    for name, k, S, word in cases:
        assert len(word) == len(S) > k and S == sorted(set(S)) and S[-1] < n
        d = em.decode(word, S, k, w, p)
        assert not d.errpos & ~sum(1 << q for q in S)
        if "phantom" in name:
            assert d.status == 2, name
        by_set.setdefault((k, tuple(S)), set()).add(d.status)
    assert {k for k, _ in by_set} == {2 * l, 3 * l, 1, n - 1}
    assert all(len(S) == n for k, S in by_set if k == n - 1)
    for (k, S), seen in by_set.items():
        if (len(S) - k) // 2 >= 1:
            assert seen == {0, 1, 2}, (k, S)
    if l == 8:
        absent = [set(range(n)) - set(S) for _, S in by_set]
        assert any(a and all(q + 16 in a for q in a if q < 16) and all(q - 16 in a for q in a if q >= 16) for a in absent)
        assert any(a and all(q % 2 for q in a) for a in absent) and any(a and not any(q % 2 for q in a) for a in absent)
