"""Bounded-distance decoding of packed shares with the extended Euclidean algorithm (Gao): an independent statement of what
zk_pss_unpack_robust computes, over any prime and any domain generator.

TEST INFRASTRUCTURE ONLY.  Polynomials are coefficient lists, lowest degree first, without trailing zeros ([] is zero).
For a received word y on the domain {omega^p : p < n} and a dimension k, cap = (n - k) // 2:
  status 0  the interpolant of y has degree < k                       -> message = the interpolant
  status 1  a polynomial of degree < k differs from y in 1 .. cap places -> that polynomial (it is unique), errpos = the places
  status 2  neither                                                   -> message zeros, errpos 0
The decoder is secret-sharing/src/gao.rs (partial_xgcd, decode_to_message) with true polynomial divisions, followed by the
three checks its todo asks for: the division r / s leaves no remainder, deg h < k, and h lies within cap of y."""
from collections import namedtuple

Decoded = namedtuple("Decoded", "status message errpos")


def inv(a, p):
    return pow(a, p - 2, p)


def trim(a):
    a = list(a)
    while a and a[-1] == 0:
        a.pop()
    return a


def degree(a):
    """ark_poly's DensePolynomial::degree: 0 for the zero polynomial"""
    return max(len(trim(a)) - 1, 0)


def poly_sub(a, b, p):
    n = max(len(a), len(b))
    a, b = list(a) + [0] * (n - len(a)), list(b) + [0] * (n - len(b))
    return trim([(x - y) % p for x, y in zip(a, b)])


def poly_mul(a, b, p):
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % p
    return trim(out)


def poly_divmod(a, b, p):
    a, b = trim(a), trim(b)
    assert b, "division by the zero polynomial"
    if len(a) < len(b):
        return [], a
    q = [0] * (len(a) - len(b) + 1)
    lc = inv(b[-1], p)
    for i in reversed(range(len(q))):
        c = a[i + len(b) - 1] * lc % p
        q[i] = c
        for j, y in enumerate(b):
            a[i + j] = (a[i + j] - c * y) % p
    return trim(q), trim(a)


def poly_eval(a, x, p):
    acc = 0
    for c in reversed(a):
        acc = (acc * x + c) % p
    return acc


def partial_xgcd(a, b, codelength, dimension, p):
    """gao.rs:11-45: Euclid on a and b until a remainder has degree < (n + k) / 2; returns (r, s)"""
    stop = (dimension + codelength) // 2
    s, prev_s = [1], []
    r, prev_r = trim(b), trim(a)
    while degree(r) >= stop:
        q, _ = poly_divmod(prev_r, r, p)
        r, prev_r = poly_sub(prev_r, poly_mul(q, r, p), p), r
        s, prev_s = poly_sub(prev_s, poly_mul(q, s, p), p), s
    return r, s


def _powers(omega, n, p):
    out = [1] * n
    for i in range(1, n):
        out[i] = out[i - 1] * omega % p
    return out


def interpolate(y, omega, p):
    """IFFT over {omega^i}: coefficients of the polynomial of degree < n through the word"""
    n = len(y)
    wi, ninv = _powers(inv(omega, p), n, p), inv(n, p)
    return trim([ninv * sum(y[q] * wi[j * q % n] for q in range(n)) % p for j in range(n)])


def encode(msg, n, omega, p):
    return [poly_eval(msg, x, p) for x in _powers(omega, n, p)]


def decode(y, k, omega, p):
    """-> Decoded(status, message padded to k coefficients, errpos)"""
    n = len(y)
    assert 1 <= k <= n - 1
    cap = (n - k) // 2
    failed = Decoded(2, [0] * k, 0)
    R = interpolate(y, omega, p)
    if len(R) <= k:
        return Decoded(0, R + [0] * (k - len(R)), 0)
    z = [p - 1] + [0] * (n - 1) + [1]
    r, s = partial_xgcd(z, R, n, k, p)
    h, rem = poly_divmod(r, s, p)
    if rem or len(h) > k:
        return failed
    code = encode(h, n, omega, p)
    errpos = sum(1 << i for i in range(n) if code[i] != y[i])
    if bin(errpos).count("1") > cap:
        return failed
    return Decoded(1, h + [0] * (k - len(h)), errpos)


def secrets(message, l, g, omega_2l, p):
    """the l secrets of a decoded message: h(g omega_2l^i), i < l"""
    return [poly_eval(message, g * pow(omega_2l, i, p) % p, p) for i in range(l)]


def brute_force(y, k, omega, p):
    """every polynomial of degree < k within cap of y, by interpolating through every k-subset (tiny fields only)"""
    from itertools import combinations
    n = len(y)
    cap = (n - k) // 2
    found = set()
    xs = [pow(omega, i, p) for i in range(n)]
    for sub in combinations(range(n), k):
        # Lagrange through the subset
        h = []
        for i in sub:
            num, den = [1], 1
            for j in sub:
                if j != i:
                    num = poly_mul(num, [(-xs[j]) % p, 1], p)
                    den = den * (xs[i] - xs[j]) % p
            c = y[i] * inv(den, p) % p
            h = trim([(a + c * b) % p for a, b in zip(h + [0] * (k - len(h)), num + [0] * (k - len(num)))])
        if sum(1 for i in range(n) if poly_eval(h, xs[i], p) != y[i]) <= cap:
            found.add(tuple(h + [0] * (k - len(h))))
    return found


# ---------------------------------------------------------------- the case list the native and GPU tests share
def case_list(l, p, omega, seed):
    """[(name, k, y)]: received words over the share domain of packing factor l covering every class of the decoder.
    Deterministic in (l, p, omega, seed)."""
    import random
    rnd = random.Random(seed * 1000 + l)
    n = 4 * l
    xs = [pow(omega, i, p) for i in range(n)]
    cases = []
    dims = sorted({2 * l, 3 * l, 4 * l - 1, 1, n - 1})
    for k in dims:
        cap = (n - k) // 2
        msg = [rnd.randrange(1, p) for _ in range(k)]
        code = encode(msg, n, omega, p)

        def corrupt(word, pos, rnd=rnd):
            w = list(word)
            for i in pos:
                w[i] = (w[i] + rnd.randrange(1, p)) % p
            return w

        for e in range(0, cap + 3):
            if e > n:
                continue
            cases.append(("k%d_e%d" % (k, e), k, corrupt(code, rnd.sample(range(n), e))))
        if cap >= 1:
            cases.append(("k%d_first" % k, k, corrupt(code, [0])))
            cases.append(("k%d_last" % k, k, corrupt(code, [n - 1])))
            w = list(code)
            w[rnd.randrange(n)] = 0
            cases.append(("k%d_tozero" % k, k, w))
            cases.append(("k%d_zeromsg_e1" % k, k, corrupt([0] * n, [rnd.randrange(n)])))
        cases.append(("k%d_zeromsg" % k, k, [0] * n))
        if cap >= 2:
            # two errors with e_a w^a + e_b w^b = 0: the top coefficient of the interpolant vanishes
            a, b = rnd.sample(range(n), 2)
            ea = rnd.randrange(1, p)
            eb = (-ea * xs[a]) % p * inv(xs[b], p) % p
            w = list(code)
            w[a] = (w[a] + ea) % p
            w[b] = (w[b] + eb) % p
            cases.append(("k%d_topzero" % k, k, w))
        if k >= 2 and cap >= 1 and n - k + 1 - cap > cap:
            # m2 = m1 + c prod_{j in S} (X - w^j), |S| = k - 1: the codewords differ in n - k + 1 places; move cap of them
            # from m2's values to m1's -> distance cap from m2, n - k + 1 - cap from m1
            S = rnd.sample(range(n), k - 1)
            prod = [rnd.randrange(1, p)]
            for j in S:
                prod = poly_mul(prod, [(-xs[j]) % p, 1], p)
            m2 = [(x + y) % p for x, y in zip(msg, prod + [0] * (k - len(prod)))]
            c2 = encode(m2, n, omega, p)
            differ = [i for i in range(n) if i not in S]
            w = list(c2)
            for i in rnd.sample(differ, cap):
                w[i] = code[i]
            cases.append(("k%d_second_codeword" % k, k, w))
        for t in range(3):
            if cap + 1 <= n:
                cases.append(("k%d_capplus1_%d" % (k, t), k, corrupt(code, rnd.sample(range(n), cap + 1))))
    return cases
