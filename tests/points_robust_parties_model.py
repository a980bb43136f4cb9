"""What zk_pss_unpack_points_robust_parties and zk_pss_repair_points_parties decide about the point shares Y_p = y_p G of a
party list, stated on the scalar word y: the verdict of the unchanged tests/gao_erasure_model.py, cut down to the one error
per chunk that can be located in the exponent, as tests/points_robust_model.py cuts tests/gao_model.py down.

TEST INFRASTRUCTURE ONLY.  Both are exact bounded-distance decoders of the code on the listed points -- Gao's up to
(|S| - k) // 2 wrong shares, the point form up to one (none when |S| - k = 1):
  status 0                                  stays 0
  status 1 with one bit in errpos           stays 1 with that bit (a party id, never an absent party)
  everything else                           is 2: message zeros, errpos 0
Also the lists and words the native and the GPU test share."""
import random

import gao_erasure_model as gem
from gao_model import Decoded, poly_eval, trim


def decode(word, parties, k, omega, p):
    """word[i]: the share of parties[i] -> Decoded(status, message padded to k coefficients, errpos by party id)"""
    d = gem.decode(word, parties, k, omega, p)
    if d.status == 0 or (d.status == 1 and bin(d.errpos).count("1") == 1):
        return d
    return Decoded(2, [0] * k, 0)


def repaired(word, parties, k, omega, p):
    """(Decoded, the compact word after zk_pss_repair_points_parties): the codeword on the listed points for status 1"""
    d = decode(word, parties, k, omega, p)
    if d.status != 1:
        return d, list(word)
    h = trim(d.message)
    return d, [poly_eval(h, pow(omega, q, p), p) for q in parties]


def lists(l):
    """[(name, parties)] at dimension k = 2l: all present; the first, a middle and the last party absent; rho = 2l - 2, the
    last list that still corrects; rho = 2l - 1, detection only"""
    n = 4 * l
    full = list(range(n))
    rnd = random.Random(900 + l)
    out = []

    def add(name, s):
        s = sorted(s)
        if all(s != t for _, t in out):
            out.append((name, s))

    add("all", full)
    for name, e in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        add("absent_" + name, [q for q in full if q != e])
    add("rho_2l_minus_2", rnd.sample(full, 2 * l + 2))
    add("rho_2l_minus_1", rnd.sample(full, 2 * l + 1))
    return out


def words(l, parties, k, omega, p, seed):
    """[(name, word on the listed points)]: clean, one error at each listed party, a wrong share that is zero, two errors"""
    rnd = random.Random(seed)
    m = len(parties)
    msg = [rnd.randrange(1, p) for _ in range(k)]
    code = [poly_eval(msg, pow(omega, q, p), p) for q in parties]

    def corrupt(pos):
        w = list(code)
        for i in pos:
            w[i] = (w[i] + rnd.randrange(1, p)) % p
        return w

    out = [("clean", list(code))]
    out += [("party%d" % parties[i], corrupt([i])) for i in range(m)]
    w = list(code)
    w[rnd.randrange(m)] = 0
    out.append(("tozero", w))
    out += [("two_%d" % t, corrupt(rnd.sample(range(m), 2))) for t in range(2)]
    return out


def case_list(l, omega, p, seed=7):
    """[(name, k, parties, word)]: every list of lists(l) with its words at k = 2l, and k = 4l - 1 with all present"""
    n = 4 * l
    cases = []
    for lname, S in lists(l):
        for wname, w in words(l, S, 2 * l, omega, p, seed * 100 + len(cases)):
            cases.append(("k%d_%s_%s" % (2 * l, lname, wname), 2 * l, S, w))
    full = list(range(n))
    for wname, w in words(l, full, n - 1, omega, p, seed * 100 + 99):
        if wname == "clean" or wname.startswith("party") and int(wname[5:]) in (0, n - 1):
            cases.append(("k%d_all_%s" % (n - 1, wname), n - 1, full, w))
    return cases
