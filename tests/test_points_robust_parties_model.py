"""tests/points_robust_parties_model.py against gao_erasure_model.brute_force on F_17 at l = 1 (n = 4, w = 4): every party list
with more than k parties, every codeword of a few messages, and every single error on it."""
from itertools import combinations, product

import gao_erasure_model as gem
import points_robust_parties_model as prpm
from gao_model import poly_eval

P, W, N = 17, 4, 4


def _lists(k):
    return [list(s) for m in range(k + 1, N + 1) for s in combinations(range(N), m)]


def _check(word, S, k):
    d = prpm.decode(word, S, k, W, P)
    found = gem.brute_force(word, S, k, W, P)           # within Gao's cap of the word
    cap = 1 if len(S) - k >= 2 else 0
    near = {m: e for m, e in found.items() if bin(e).count("1") <= cap}
    if d.status == 2:
        assert not near, (word, S, k)
        assert d.message == [0] * k and d.errpos == 0
        return d
    assert near == {tuple(d.message): d.errpos}, (word, S, k)
    assert d.status == (1 if d.errpos else 0)
    assert all((d.errpos >> q) & 1 == 0 for q in range(N) if q not in S)
    return d


def test_every_list_and_every_single_error():
    assert pow(W, N, P) == 1 and pow(W, N // 2, P) != 1
    seen = set()
    for k in (1, 2, 3):
        for S in _lists(k):
            xs = [pow(W, q, P) for q in S]
            for msg in product((0, 1, 5, 16), repeat=k):
                code = [poly_eval(list(msg), x, P) for x in xs]
                d = _check(code, S, k)
                assert (d.status, tuple(d.message)) == (0, msg)
                for i in range(len(S)):
                    for e in (1, 7, 16):
                        word = list(code)
                        word[i] = (word[i] + e) % P
                        d = _check(word, S, k)
                        seen.add(d.status)
                        if len(S) - k >= 2:
                            assert (d.status, d.errpos, tuple(d.message)) == (1, 1 << S[i], msg)
                            fixed = prpm.repaired(word, S, k, W, P)[1]
                            assert fixed == code
                        else:
                            assert d.status == 2 and prpm.repaired(word, S, k, W, P)[1] == word
    assert seen == {1, 2}


def test_two_errors_never_name_an_absent_party():
    k = 2
    for S in _lists(k):
        xs = [pow(W, q, P) for q in S]
        code = [poly_eval([3, 11], x, P) for x in xs]
        for i, j in combinations(range(len(S)), 2):
            for ei, ej in product((1, 9), (2, 16)):
                word = list(code)
                word[i] = (word[i] + ei) % P
                word[j] = (word[j] + ej) % P
                _check(word, S, k)
