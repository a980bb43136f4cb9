"""Bounded-distance decoding of the packed shares of a party list: an independent statement of what
zk_pss_unpack_robust_parties computes, over any prime and any domain generator.

TEST INFRASTRUCTURE ONLY.  The shares of the listed parties S (ascending ids below n) are a word on the points
{omega^p : p in S}; the other parties are absent.  With k the dimension and cap = (|S| - k) // 2:
  status 0  the interpolant through the listed points has degree < k                -> message = the interpolant
  status 1  a polynomial of degree < k differs from the word in 1 .. cap places      -> that polynomial (it is unique),
            errpos = the ids of those parties (bit p for party p, never an absent one)
  status 2  neither                                                                 -> message zeros, errpos 0
Nothing here extends the word to the full domain: the interpolation is Lagrange's over the listed points with the polynomial
arithmetic of gao_model, the decoder is Gao's over g_0 = prod_{p in S} (X - omega^p) (gao.rs partial_xgcd with |S| as the code
length, stopping at the first remainder of degree < (|S| + k) / 2), followed by the three checks of gao_model.decode."""
import functools
from itertools import combinations

import gao_model as gm
from gao_model import Decoded, inv, poly_divmod, poly_eval, poly_mul, trim


def vanishing(xs, p):
    g0 = [1]
    for x in xs:
        g0 = poly_mul(g0, [(-x) % p, 1], p)
    return g0


def interpolate_on(xs, ys, p):
    """coefficients of the polynomial of degree < len(xs) through (xs[i], ys[i])"""
    out = [0] * len(xs)
    for y, basis in zip(ys, _lagrange(tuple(xs), p)[1]):
        if y:
            for j, v in enumerate(basis):
                out[j] = (out[j] + y * v) % p
    return trim(out)


@functools.lru_cache(maxsize=64)
def _lagrange(xs, p):
    """(g_0, the Lagrange basis polynomials g_0 / ((X - x_i) g_0'(x_i))) of the points xs: a party list's, computed once"""
    g0 = vanishing(xs, p)
    basis = []
    for x in xs:
        qi, rem = poly_divmod(g0, [(-x) % p, 1], p)
        assert not rem
        c = inv(poly_eval(qi, x, p), p)
        basis.append([c * v % p for v in qi])
    return g0, basis


def decode(word, parties, k, omega, p):
    """word[i]: the share of party parties[i] -> Decoded(status, message padded to k coefficients, errpos by party id)"""
    m = len(parties)
    assert list(parties) == sorted(set(parties)) and len(word) == m and 1 <= k < m
    cap = (m - k) // 2
    failed = Decoded(2, [0] * k, 0)
    xs = [pow(omega, q, p) for q in parties]
    R = interpolate_on(xs, word, p)
    if len(R) <= k:
        return Decoded(0, R + [0] * (k - len(R)), 0)
    r, s = gm.partial_xgcd(_lagrange(tuple(xs), p)[0], R, m, k, p)
    h, rem = poly_divmod(r, s, p)
    if rem or len(h) > k:
        return failed
    errpos = sum(1 << q for q, x, y in zip(parties, xs, word) if poly_eval(h, x, p) != y)
    if bin(errpos).count("1") > cap:
        return failed
    return Decoded(1, h + [0] * (k - len(h)), errpos)


def brute_force(word, parties, k, omega, p):
    """{message: errpos} of every polynomial of degree < k within cap of the word, through every k-subset (tiny fields only)"""
    m = len(parties)
    cap = (m - k) // 2
    xs = [pow(omega, q, p) for q in parties]
    found = {}
    for sub in combinations(range(m), k):
        h = interpolate_on([xs[i] for i in sub], [word[i] for i in sub], p)
        err = sum(1 << parties[i] for i in range(m) if poly_eval(h, xs[i], p) != word[i])
        if bin(err).count("1") <= cap:
            found[tuple(h + [0] * (k - len(h)))] = err
    return found


# ---------------------------------------------------------------- the case list the native and GPU tests share
def party_sets(l, k, rnd):
    """[(name, parties)] for dimension k: every set has more than k parties"""
    n = 4 * l
    full = list(range(n))
    sets = []

    def add(name, s):
        s = sorted(s)
        if len(s) > k and all(s != t for _, t in sets):
            sets.append((name, s))

    add("all", full)
    if k == n - 1:
        return sets
    for name, e in (("first", 0), ("last", n - 1), ("middle", n // 2)):
        add("absent_" + name, [q for q in full if q != e])
    add("contig_k1", range(k + 1))                                  # cap 0: detection only
    add("scatter_k1", rnd.sample(full, k + 1))
    add("contig_k2", range(n - k - 2, n))                           # the largest rho with cap >= 1
    add("scatter_k2", rnd.sample(full, k + 2))
    if k + 3 <= n:
        add("scatter_k3", rnd.sample(full, k + 3))                  # the floor in cap
        add("contig_k3", [(5 + i) % n for i in range(k + 3)])       # (wraps round the domain)
    if l == 8:
        # absent p and p + 16 meet in the first decimation stage of the two-lane split
        add("absent_3_19", [q for q in full if q not in (3, 19)])
        add("absent_5_21_10_26", [q for q in full if q not in (5, 21, 10, 26)])
        # all absent parties of one parity: one lane of the split loses nothing
        add("absent_odd", [q for q in full if q not in (1, 7, 13, 29)])
        add("absent_even", [q for q in full if q not in (0, 12, 30)])
    return sets


def case_list_parties(l, p, omega, seed):
    """[(name, k, parties, word_on_S)]: words over the listed points covering every class of the decoder with absent parties.
    Deterministic in (l, p, omega, seed)."""
    import random
    rnd = random.Random(seed * 1000 + l)
    n = 4 * l
    cases = []
    for k in sorted({2 * l, 3 * l, 1, n - 1}):
        for sname, S in party_sets(l, k, rnd):
            m = len(S)
            cap = (m - k) // 2
            absent = [q for q in range(n) if q not in S]
            xs = [pow(omega, q, p) for q in S]
            msg = [rnd.randrange(1, p) for _ in range(k)]
            code = [poly_eval(msg, x, p) for x in xs]
            tag = "k%d_%s_" % (k, sname)

            def put(name, word):
                cases.append((tag + name, k, list(S), list(word)))

            def corrupt(word, pos):
                w = list(word)
                for i in pos:
                    w[i] = (w[i] + rnd.randrange(1, p)) % p
                return w

            for e in range(0, cap + 3):
                if e <= m:
                    put("e%d" % e, corrupt(code, rnd.sample(range(m), e)))
            put("zeromsg", [0] * m)
            if cap >= 1:
                put("first", corrupt(code, [0]))
                put("last", corrupt(code, [m - 1]))
                near = [i for i, q in enumerate(S) if (q + 1) % n in absent or (q - 1) % n in absent]
                if near:
                    put("next_to_absent", corrupt(code, [rnd.choice(near)]))
                w = list(code)
                w[rnd.randrange(m)] = 0
                put("tozero", w)
                put("zeromsg_e1", corrupt([0] * m, [rnd.randrange(m)]))
            if cap >= 2:
                # two errors with e_a / g0'(x_a) + e_b / g0'(x_b) = 0: the top coefficient of the interpolant through S vanishes
                a, b = rnd.sample(range(m), 2)
                da, db = 1, 1
                for j in range(m):
                    if j != a:
                        da = da * (xs[a] - xs[j]) % p
                    if j != b:
                        db = db * (xs[b] - xs[j]) % p
                ea = rnd.randrange(1, p)
                eb = (-ea) % p * inv(da, p) % p * db % p
                w = list(code)
                w[a] = (w[a] + ea) % p
                w[b] = (w[b] + eb) % p
                put("topzero", w)
            if k >= 2 and cap >= 1 and m - k + 1 - cap > cap:
                # m2 = m1 + c prod_{j in Z} (X - x_j), |Z| = k - 1 listed points: the codewords differ in m - k + 1 places;
                # move cap of them from m2's values to m1's -> distance cap from m2, m - k + 1 - cap from m1
                Z = rnd.sample(range(m), k - 1)
                prod = [rnd.randrange(1, p)]
                for j in Z:
                    prod = poly_mul(prod, [(-xs[j]) % p, 1], p)
                m2 = [(x + y) % p for x, y in zip(msg, prod + [0] * (k - len(prod)))]
                c2 = [poly_eval(m2, x, p) for x in xs]
                w = list(c2)
                for i in rnd.sample([i for i in range(m) if i not in Z], cap):
                    w[i] = code[i]
                put("second_codeword", w)
            for t in range(3):
                if cap + 1 <= m:
                    put("capplus1_%d" % t, corrupt(code, rnd.sample(range(m), cap + 1)))
            if absent and cap >= 1:
                # phantom: y = h' / Lambda on S with deg h' < k + rho and h' zero at all absent points but one -- a decoder
                # that works on the full domain with zeros at the absent places finds h' one "error" away, at an absent party
                keep = rnd.choice(absent)
                hp = [rnd.randrange(1, p) for _ in range(k + 1)]
                for e in absent:
                    if e != keep:
                        hp = poly_mul(hp, [(-pow(omega, e, p)) % p, 1], p)
                lam = vanishing([pow(omega, e, p) for e in absent], p)
                put("phantom", [poly_eval(hp, x, p) * inv(poly_eval(lam, x, p), p) % p for x in xs])
    return cases
