"""Points inside and outside the order-r subgroups of BN254 and BLS12-381, with their ground truth, for the subgroup tests
(test_native_subgroup.py, test_gpu_subgroup.py, test_gpu_verify_bytes.py).  Not a test module.

Ground truth of every verdict is "[r]P = O" with the oracle's group law.  `oracle.curve.Group.mul` reduces its scalar mod
r, so the multiplications here are an unreduced double-and-add over `Group.double` / `Group.add`.  Random points of the
twist need a square root in Fq2, which the oracle has not: q = 3 mod 4 on both curves (Adj, Rodriguez-Henriquez, Alg. 9).

Cofactor-torsion points of prime order l: with n the (hard-coded, checked) order of the curve or twist, strip the full
power of l from n to get m, take T = [m]Q for a random curve point Q, and multiply T by l while [l]T != O."""
import functools
import random

from oracle.curve import g1, g2
from oracle.params import BLS12_381, BN254, CURVES

BN_X = 4965661367192848881
BLS_X = -0xD201000000010000

# group orders: #E(Fq) = q + 1 - t; the sextic twist's from the CM equation -- as the cofactor formulas of the families
ORDER = {
    ("bn254", 1): BN254.r,
    ("bn254", 2): BN254.r * (2 * BN254.q - BN254.r),
    ("bls12_381", 1): BLS12_381.r * ((BLS_X - 1) ** 2 // 3),
    ("bls12_381", 2): BLS12_381.r * ((BLS_X ** 8 - 4 * BLS_X ** 7 + 5 * BLS_X ** 6 - 4 * BLS_X ** 4 + 6 * BLS_X ** 3
                                      - 4 * BLS_X ** 2 - 4 * BLS_X + 13) // 9),
}
# small primes dividing the cofactors (trial division)
TORSION_PRIMES = {
    ("bn254", 1): (),
    ("bn254", 2): (10069,),
    ("bls12_381", 1): (3, 11, 10177),
    ("bls12_381", 2): (13, 23, 2713, 11953, 262069),
}


def group(curve, grp):
    c = CURVES[curve]
    return g1(c) if grp == 1 else g2(c)


def umul(G, P, k):
    """[k]P, Jacobian, k a non-negative integer taken as it is"""
    R = G.identity
    if k == 0:
        return R
    for bit in bin(k)[2:]:
        R = G.double(R)
        if bit == "1":
            R = G.add(R, P)
    return R


def f2_pow(F, a, e):
    r = F.one
    while e:
        if e & 1:
            r = F.mul(r, a)
        a = F.mul(a, a)
        e >>= 1
    return r


def f2_sqrt(F, a):
    """a square root of a in Fq2 = Fq[u]/(u^2 + 1), q = 3 mod 4, or None"""
    q = F.q
    assert q % 4 == 3 and F.nr == q - 1
    if F.is_zero(a):
        return a
    a1 = f2_pow(F, a, (q - 3) // 4)
    alpha = F.mul(F.mul(a1, a1), a)
    if F.mul((alpha[0], (-alpha[1]) % q), alpha) == (q - 1, 0):
        return None
    x0 = F.mul(a1, a)
    x = F.mul((0, 1), x0) if alpha == (q - 1, 0) else F.mul(f2_pow(F, F.add(alpha, F.one), (q - 1) // 2), x0)
    return x if F.mul(x, x) == a else None


def rhs(G, x):
    F = G.F
    return F.add(F.mul(F.sqr(x), x), G.b)


def random_curve_point(G, rnd, grp):
    """an affine point of the whole curve / twist (almost never in the subgroup where the cofactor is not 1)"""
    q = G.F.q
    while True:
        x = rnd.randrange(q) if grp == 1 else (rnd.randrange(q), rnd.randrange(q))
        y = G.F.sqrt(rhs(G, x)) if grp == 1 else f2_sqrt(G.F, rhs(G, x))
        if y is not None:
            if rnd.randrange(2):
                y = G.F.neg(y)
            assert G.on_curve((x, y))
            return (x, y)


def torsion_point(G, rnd, grp, n, ell):
    m = n
    while m % ell == 0:
        m //= ell
    while True:
        T = umul(G, G.from_affine(random_curve_point(G, rnd, grp)), m)
        if G.is_identity(T):
            continue
        while not G.is_identity(umul(G, T, ell)):
            T = umul(G, T, ell)
        return G.to_affine(T)


def in_subgroup(G, p):
    """ground truth for an affine point of the curve (None: the identity)"""
    return p is None or G.is_identity(umul(G, G.from_affine(p), G.r))


def flat(p, grp):
    """affine oracle point -> its 2 or 4 base-field coordinates (None -> zeros)"""
    if p is None:
        return [0] * (2 * grp)
    return [p[0], p[1]] if grp == 1 else [p[0][0], p[0][1], p[1][0], p[1][1]]


@functools.lru_cache(maxsize=None)
def classes(curve, grp):
    """dict class name -> list of (affine point, in the subgroup?) over points of the curve.  Built once per group."""
    G = group(curve, grp)
    rnd = random.Random(0x5B + 2 * len(curve) + grp)
    n = ORDER[(curve, grp)]
    gen = G.from_affine(G.gen)
    probe = random_curve_point(G, rnd, grp)
    assert G.is_identity(umul(G, G.from_affine(probe), n)), "hard-coded group order"
    out = {}
    out["generator"] = [G.gen]
    out["multiples"] = [G.to_affine(umul(G, gen, rnd.randrange(1, G.r))) for _ in range(16)]
    out["identity"] = [None]
    out["curve"] = [random_curve_point(G, rnd, grp) for _ in range(16)]
    out["r_times"] = [G.to_affine(umul(G, G.from_affine(random_curve_point(G, rnd, grp)), G.r))]
    tors = [torsion_point(G, rnd, grp, n, ell) for ell in TORSION_PRIMES[(curve, grp)]]
    for ell, t in zip(TORSION_PRIMES[(curve, grp)], tors):
        assert t is not None and G.is_identity(umul(G, G.from_affine(t), ell))
    out["torsion"] = tors
    out["gen_plus_torsion"] = [G.to_affine(G.add(gen, G.from_affine(t))) for t in tors]
    res = {k: [(p, in_subgroup(G, p)) for p in v] for k, v in out.items()}
    # what the construction promises, so that a test cannot pass on an empty class
    assert all(ok for _, ok in res["generator"] + res["multiples"] + res["identity"])
    assert not any(ok for _, ok in res["torsion"] + res["gen_plus_torsion"])
    if TORSION_PRIMES[(curve, grp)]:
        assert not any(ok for _, ok in res["curve"])
        assert not any(ok for p, ok in res["r_times"] if p is not None)
    return res


def off_curve(curve, grp):
    """the generator with y + 1: canonical coordinates, not on the curve"""
    G = group(curve, grp)
    x, y = G.gen
    p = (x, G.F.add(y, G.F.one))
    assert not G.on_curve(p)
    return p
