"""The verifier on the device (`pytest -m gpu`): zk_multi_pairing, zk_fq12_selftest and zk_groth16_verify against the
golden pairing value of the reference's fixture, oracle.pairing and device-only identities.  Everything is an integer:
every comparison is exact equality.  The Python oracle takes ~0.35 s per pairing, so oracle-checked cases are a handful
per curve and bilinearity carries the breadth."""
import functools
import json
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import groth16 as zg
from zksaas_amd.api import ZK_G1, ZK_G2, DeviceBuffer, fq12_selftest, multi_pairing
from oracle import pairing as op
from oracle.curve import g1, g2
from oracle.params import BN254, CURVES
from oracle.prng import rand_fp

from gpu_util import ctx, enc_affine
from test_pairing import _small_r1cs_mod

HERE = os.path.dirname(os.path.abspath(__file__))
BOTH = ["bn254", "bls12_381"]
GROUPS_PER_WAVE = 8            # 64 lanes / 8 lanes per Fq12 value
GROUPS_PER_BLOCK = 32          # 256 threads


def flat12(f):
    return [a for h in f for b in h for a in b]


def unflat12(v):
    return tuple(tuple((v[6 * h + 2 * b], v[6 * h + 2 * b + 1]) for b in range(3)) for h in range(2))


def up12(pp, vals):
    """list of oracle Fq12 -> device [len][12] Fq"""
    return DeviceBuffer.from_numpy(pp, pp.fq.encode([c for f in vals for c in flat12(f)]))


def down12(pp, buf, count):
    v = pp.fq.decode(buf.to_numpy()[:count * 12 * pp.fq.nl])
    return [unflat12(v[12 * i:12 * i + 12]) for i in range(count)]


def raw12(pp, buf, count):
    return buf.to_numpy()[:count * 12 * pp.fq.nl].reshape(count, 12 * pp.fq.nl)


def pair_dev(pp, P, Q, k=1):
    """oracle affine points (None = identity) -> zk_multi_pairing -> list of oracle Fq12"""
    count = len(P) // k
    out = multi_pairing(pp, DeviceBuffer.from_numpy(pp, enc_affine(pp, P)), DeviceBuffer.from_numpy(pp, enc_affine(pp, Q, True)),
                        k, count)
    return down12(pp, out, count)


def test_golden_pairing_value_of_the_reference_fixture():
    """e(vk_alpha_1, vk_beta_2) of tests/golden/verification_key_bn254.json equals the file's vk_alphabeta_12."""
    with open(os.path.join(HERE, "golden", "verification_key_bn254.json")) as fh:
        d = json.load(fh)
    alpha = (int(d["vk_alpha_1"][0]), int(d["vk_alpha_1"][1]))
    b = d["vk_beta_2"]
    beta = ((int(b[0][0]), int(b[0][1])), (int(b[1][0]), int(b[1][1])))
    gold = tuple(tuple(tuple(int(x) for x in b_) for b_ in c) for c in d["vk_alphabeta_12"])
    assert pair_dev(ctx("bn254"), [alpha], [beta]) == [gold]


@pytest.mark.parametrize("curve", BOTH)
def test_pairing_equals_the_oracle(curve):
    """4 pairs (a G1, b G2) with random a, b; one k = 3 group against multi_pairing."""
    c = CURVES[curve]
    pp, G1, G2, pr = ctx(curve), g1(c), g2(c), op.pairing_for(c)
    P = [G1.to_affine(G1.mul(G1.from_affine(c.g1), rand_fp(301, i, c.r))) for i in range(4)]
    Q = [G2.to_affine(G2.mul(G2.from_affine(c.g2), rand_fp(302, i, c.r))) for i in range(4)]
    assert pair_dev(pp, P, Q) == [pr.pairing(p, q) for p, q in zip(P, Q)]
    assert pair_dev(pp, P[1:], Q[1:], k=3) == [pr.multi_pairing(list(zip(P[1:], Q[1:])))]


# ---------------------------------------------------------------------------------------------------- the tower
@functools.lru_cache(maxsize=None)
def _frob_coeff(curve, j, k):
    pr = op.pairing_for(CURVES[curve])
    return pr.T.pow2(pr.T.xi, j * (pr.q ** k - 1) // 6)


def _frob_ref(pr, a, k):
    """a^(q^k) from Tower's own Fq2 operations: conj^k of each w-basis coefficient times XI^(j (q^k - 1) / 6)"""
    T, q = pr.T, pr.q
    out = [[None] * 3, [None] * 3]
    for j in range(6):
        x = a[j % 2][j // 2]
        if k & 1:
            x = T.conj2(x)
        out[j % 2][j // 2] = T.mul2(x, _frob_coeff(pr.curve.name, j, k))
    return (tuple(out[0]), tuple(out[1]))


@functools.lru_cache(maxsize=None)
def _tower_cases(curve):
    """33 inputs (two workgroups) and, per op, the oracle's results -- computed once per curve"""
    c = CURVES[curve]
    pr = op.pairing_for(c)
    T, q = pr.T, c.q
    rnd = random.Random(0x7A + len(curve))
    n = GROUPS_PER_BLOCK + 1
    a = [unflat12([rnd.randrange(q) for _ in range(12)]) for _ in range(n)]
    b = [unflat12([rnd.randrange(q) for _ in range(12)]) for _ in range(n)]
    a[2], a[3], a[4] = unflat12([q - 1] * 12), T.one12, unflat12([0, 1] * 6)
    z = T.zero2
    line = lambda f: ((f[0][0], z, z), (f[0][1], f[0][2], z)) if pr.twist == "D" else ((f[0][0], f[0][1], z), (z, f[0][2], z))
    for k in (1, 2, 3):                                  # the Fq2-level reference is the oracle's own power
        assert _frob_ref(pr, a[0], k) == T.pow12(a[0], q ** k)
    seeds = []
    for x in a[:3]:                                      # into the cyclotomic subgroup
        e = T.mul12(T.conj12(x), T.inv12(x))
        seeds.append(T.mul12(_frob_ref(pr, e, 2), e))
    cyc = list(seeds)
    while len(cyc) < n:                                  # products of cyclotomic elements are cyclotomic
        cyc.append(T.mul12(cyc[-1], cyc[-3]))
    want = {
        "mul": [T.mul12(x, y) for x, y in zip(a, b)],
        "sqr": [T.mul12(x, x) for x in a],
        "inverse": [T.inv12(x) for x in a],
        "conj": [T.conj12(x) for x in a],
        "frobenius1": [_frob_ref(pr, x, 1) for x in a],
        "frobenius2": [_frob_ref(pr, x, 2) for x in a],
        "frobenius3": [_frob_ref(pr, x, 3) for x in a],
        "cyclotomic_sqr": [T.mul12(x, x) for x in cyc],
        "line_mul": [T.mul12(x, line(y)) for x, y in zip(a, b)],
    }
    return a, b, cyc, want


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("op_name", ["mul", "sqr", "inverse", "conj", "frobenius1", "frobenius2", "frobenius3",
                                     "cyclotomic_sqr", "line_mul"])
def test_lane_split_tower_equals_the_oracle_tower(curve, op_name):
    """zk_fq12_selftest at len = 1, the lane groups of a wave -1 / exact / +1, and one more than a workgroup holds."""
    pp = ctx(curve)
    a, b, cyc, want = _tower_cases(curve)
    src = cyc if op_name == "cyclotomic_sqr" else a
    for ln in (1, GROUPS_PER_WAVE - 1, GROUPS_PER_WAVE, GROUPS_PER_WAVE + 1, GROUPS_PER_BLOCK + 1):
        out = fq12_selftest(pp, op_name, up12(pp, src[:ln]), up12(pp, b[:ln]), ln)
        assert down12(pp, out, ln) == want[op_name][:ln], (op_name, ln)


# ---------------------------------------------------------------------------------------- device-only identities
NCASE = 65


@functools.lru_cache(maxsize=None)
def _points(curve):
    """65 random (a, b): device buffers of a P, a b P, P (G1) and b Q, a b Q, Q (G2), and E1 = e(a P, b Q)"""
    c = CURVES[curve]
    pp = ctx(curve)
    a = [rand_fp(311, i, c.r) for i in range(NCASE)]
    b = [rand_fp(312, i, c.r) for i in range(NCASE)]
    ab = [x * y % c.r for x, y in zip(a, b)]
    one = [1] * NCASE
    pts = {"aP": zg.base_points(pp, ZK_G1, pp.upload_fr(a), NCASE), "abP": zg.base_points(pp, ZK_G1, pp.upload_fr(ab), NCASE),
           "P": zg.base_points(pp, ZK_G1, pp.upload_fr(one), NCASE), "bQ": zg.base_points(pp, ZK_G2, pp.upload_fr(b), NCASE),
           "abQ": zg.base_points(pp, ZK_G2, pp.upload_fr(ab), NCASE), "Q": zg.base_points(pp, ZK_G2, pp.upload_fr(one), NCASE)}
    e1 = raw12(pp, multi_pairing(pp, pts["aP"], pts["bQ"], 1, NCASE), NCASE)
    return pts, e1


def _one_raw(pp):
    return pp.fq.encode([1] + [0] * 11).reshape(-1)


@pytest.mark.parametrize("curve", BOTH)
def test_bilinearity_on_64_random_cases(curve):
    pp = ctx(curve)
    pts, e1 = _points(curve)
    assert not any(np.array_equal(e1[i], _one_raw(pp)) for i in range(NCASE)) and len({e.tobytes() for e in e1}) == NCASE
    assert np.array_equal(raw12(pp, multi_pairing(pp, pts["abP"], pts["Q"], 1, NCASE), NCASE), e1)
    assert np.array_equal(raw12(pp, multi_pairing(pp, pts["P"], pts["abQ"], 1, NCASE), NCASE), e1)


@pytest.mark.parametrize("curve", BOTH)
def test_every_slot_equals_the_pair_computed_alone(curve):
    """count = 1, lane groups per wave -1 / exact / +1 and 65: the same values as the count = 65 run, and every one of
    the 65 slots equals a count = 1 call on that pair."""
    pp = ctx(curve)
    pts, e1 = _points(curve)
    for count in (1, GROUPS_PER_WAVE - 1, GROUPS_PER_WAVE, GROUPS_PER_WAVE + 1):
        assert np.array_equal(raw12(pp, multi_pairing(pp, pts["aP"], pts["bQ"], 1, count), count), e1[:count]), count
    w1, w2 = 2 * pp.fq.nbytes, 4 * pp.fq.nbytes
    for i in range(NCASE):
        alone = multi_pairing(pp, pts["aP"].view(i * w1, w1), pts["bQ"].view(i * w2, w2), 1, 1)
        assert np.array_equal(raw12(pp, alone, 1)[0], e1[i]), i


@pytest.mark.parametrize("curve", BOTH)
def test_inverse_pairs_and_identities_give_one(curve):
    pp = ctx(curve)
    pts, _ = _points(curve)
    nl, n = pp.fq.nl, NCASE - 1
    aP = pts["aP"].to_numpy().reshape(NCASE, 2 * nl)[:n]
    bQ = pts["bQ"].to_numpy().reshape(NCASE, 4 * nl)[:n]
    y = pp.fq.decode(aP[:, nl:])
    neg = aP.copy()
    neg[:, nl:] = pp.fq.encode([(-v) % pp.fq.p for v in y])
    P2 = np.stack([aP, neg], axis=1)                         # [n][2]: (a P, -a P)
    Q2 = np.stack([bQ, bQ], axis=1)
    out = multi_pairing(pp, DeviceBuffer.from_numpy(pp, P2), DeviceBuffer.from_numpy(pp, Q2), 2, n)
    assert all(np.array_equal(r, _one_raw(pp)) for r in raw12(pp, out, n))
    zp, zq = np.zeros_like(aP), np.zeros_like(bQ)
    for P, Q in ((zp, bQ), (aP, zq), (zp, zq)):
        out = multi_pairing(pp, DeviceBuffer.from_numpy(pp, P), DeviceBuffer.from_numpy(pp, Q), 1, n)
        assert all(np.array_equal(r, _one_raw(pp)) for r in raw12(pp, out, n))


@pytest.mark.parametrize("curve", BOTH)
def test_product_of_three_equals_the_product_of_the_singles(curve):
    pp = ctx(curve)
    pts, e1 = _points(curve)
    ng = NCASE // 3
    got = raw12(pp, multi_pairing(pp, pts["aP"], pts["bQ"], 3, ng), ng)
    col = lambda j: DeviceBuffer.from_numpy(pp, np.ascontiguousarray(e1[j:3 * ng:3]))
    prod = fq12_selftest(pp, "mul", fq12_selftest(pp, "mul", col(0), col(1), ng), col(2), ng)
    assert np.array_equal(got, raw12(pp, prod, ng))


# --------------------------------------------------------------------------------------------------- the verifier
def _decode_proof(pp, aff):
    v = pp.fq.decode(np.asarray(aff).reshape(-1, pp.fq.nl))
    return (v[0], v[1]), ((v[2], v[3]), (v[4], v[5])), (v[6], v[7])


@functools.lru_cache(maxsize=None)
def _proofs(curve):
    """five proofs of test_pairing._small_r1cs_mod (different r, s), reconstructed from all parties"""
    c = CURVES[curve]
    P = c.r
    r1, w = _small_r1cs_mod(P)
    pp = ctx(curve)
    setup = zg.SetupScalars(curve, r1, *[rand_fp(320, i, P) for i in range(5)])
    crs = zg.Crs(pp, setup)
    wit = zg.Witness(pp, curve, r1, w, seed=5)
    shares = [zg.prove(pp, crs, wit, rand_fp(321, i, P), rand_fp(322, i, P), seed=9 + i) for i in range(5)]
    affs = [zg.reconstruct(pp, sh, want_bytes=False)[0] for sh in shares]
    vk = zg.verifying_key(pp, setup)
    return pp, c, w, vk, zg.PreparedVk(pp, vk), shares, affs


@pytest.mark.parametrize("curve", BOTH)
def test_verify_accepts_reconstructed_proofs_also_from_a_party_subset(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    assert zg.verify(pp, pvk, [affs[0]], [[w[1]]]) == [True]
    present = [0, 1, 2, 4, 5, 6, 7]                              # one party dropped (lagrange_unpack)
    sub, _ = zg.reconstruct(pp, tuple(x[present] for x in shares[1]), parties=present, want_bytes=False)
    assert zg.verify(pp, pvk, [sub], [[w[1]]]) == [True]
    assert zg.verify(pp, pvk, affs, [[w[1]]] * 5) == [True] * 5


@pytest.mark.parametrize("curve", BOTH)
def test_verify_rejects_a_wrong_input_and_a_replaced_point(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    assert zg.verify(pp, pvk, [affs[0]], [[(w[1] + 1) % c.r]]) == [False]
    nl = pp.fq.nl
    bad = affs[0].copy()
    bad[:2 * nl] = affs[1][:2 * nl]                              # A replaced by another point of the curve
    assert zg.verify(pp, pvk, [bad, affs[0]], [[w[1]]] * 2) == [False, True]


@pytest.mark.parametrize("curve", BOTH)
def test_verify_batch_with_swapped_c_equals_the_oracle_proof_by_proof(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    nl = pp.fq.nl
    batch = [a.copy() for a in affs]
    batch[1][6 * nl:], batch[3][6 * nl:] = affs[3][6 * nl:], affs[1][6 * nl:]
    ovk = op.VerifyingKey(vk["alpha_g1"], vk["beta_g2"], vk["gamma_g2"], vk["delta_g2"], vk["gamma_abc_g1"])
    want = [op.verify_proof(c, ovk, _decode_proof(pp, a), [w[1]], g1(c)) for a in batch]
    assert want == [True, False, True, False, True]
    assert zg.verify(pp, pvk, batch, [[w[1]]] * 5) == want


@pytest.mark.parametrize("curve", BOTH)
def test_verify_off_curve_point_fails_that_proof_only(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    nl = pp.fq.nl
    for lo in (nl, 5 * nl, 7 * nl):                              # y of A, y.c1 of B, y of C
        bad = affs[2].copy()
        v = pp.fq.decode(bad[lo:lo + nl])[0]
        bad[lo:lo + nl] = pp.fq.encode_one((v + 1) % c.q)
        assert zg.verify(pp, pvk, [affs[0], bad, affs[1]], [[w[1]]] * 3) == [True, False, True]


@pytest.mark.parametrize("curve", BOTH)
def test_verify_with_several_public_inputs(curve):
    """Four public inputs per proof, 0, 1, r - 1 and values with every bit pattern among them.  Key and "proofs" are built
    from known discrete logs: alpha = a G1, beta = b G2, gamma = g G2, delta = d G2, abc_i = c_i G1, C = c G1, B = v G2 and
    A = u G1 with u v = a b + (c_0 + sum x_i c_i) g + c d (mod r), which is exactly the verification equation."""
    c = CURVES[curve]
    pp, r = ctx(curve), c.r
    nl = pp.fq.nl
    a, b, g, d = (rand_fp(330, i, r) for i in range(4))
    cs = [rand_fp(331, i, r) for i in range(5)]
    xs = [[0, 1, r - 1, rand_fp(332, 0, r)], [rand_fp(332, i, r) for i in range(1, 5)],
          [(1 << 64) - 1, ((1 << 128) - 1) << 64, r - 2, 2], [0, 0, 0, 0]]
    n = len(xs)
    cc = [rand_fp(333, i, r) for i in range(n)]
    vv = [rand_fp(334, i, r) for i in range(n)]
    uu = [(a * b + (cs[0] + sum(x * k for x, k in zip(xv, cs[1:]))) * g + cc[i] * d) * pow(vv[i], -1, r) % r
          for i, xv in enumerate(xs)]
    g1pts = zg.base_points(pp, ZK_G1, pp.upload_fr([a] + cs + uu + cc), 6 + 2 * n).to_numpy().reshape(-1, 2 * nl)
    g2pts = zg.base_points(pp, ZK_G2, pp.upload_fr([b, g, d] + vv), 3 + n).to_numpy().reshape(-1, 4 * nl)
    dec1 = lambda row: tuple(pp.fq.decode(row.reshape(2, nl)))
    dec2 = lambda row: (lambda v: ((v[0], v[1]), (v[2], v[3])))(pp.fq.decode(row.reshape(4, nl)))
    vk = {"alpha_g1": dec1(g1pts[0]), "gamma_abc_g1": [dec1(g1pts[1 + i]) for i in range(5)],
          "beta_g2": dec2(g2pts[0]), "gamma_g2": dec2(g2pts[1]), "delta_g2": dec2(g2pts[2])}
    pvk = zg.PreparedVk(pp, vk)
    proofs = [np.concatenate([g1pts[6 + i], g2pts[3 + i], g1pts[6 + n + i]]) for i in range(n)]
    assert zg.verify(pp, pvk, proofs, xs) == [True] * n
    for i in range(n):                                   # one input of proof i changed: that proof fails, the others hold
        bad = [list(x) for x in xs]
        bad[i][i] = (bad[i][i] + 1) % r
        assert zg.verify(pp, pvk, proofs, bad) == [j != i for j in range(n)], i
    # the oracle agrees on one of them
    ovk = op.VerifyingKey(vk["alpha_g1"], vk["beta_g2"], vk["gamma_g2"], vk["delta_g2"], vk["gamma_abc_g1"])
    assert op.verify_proof(c, ovk, _decode_proof(pp, proofs[0]), xs[0], g1(c))


@pytest.mark.parametrize("curve", BOTH)
def test_verify_wrong_input_count_is_bad_input(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    for xs in ([], [w[1], w[1]]):
        with pytest.raises(zk.ZkError) as e:
            zg.verify(pp, pvk, [affs[0]], [xs])
        assert e.value.code == 4 and "malformed verifying key" in e.value.msg


def test_bls12_377_has_no_pairing_parameters():
    pp = ctx("bls12_377")
    buf = DeviceBuffer(pp, 12 * pp.fq.nbytes)
    for call in (lambda: multi_pairing(pp, buf, buf, 1, 1), lambda: fq12_selftest(pp, "sqr", buf, None, 1),
                 lambda: zg.verify(pp, type("V", (), {"h": None})(), [np.zeros(8 * pp.fq.nl, dtype=np.uint64)], [[1]])):
        with pytest.raises(zk.ZkError) as e:
            call()
        assert e.value.code == 4 and "no pairing parameters" in e.value.msg
    with pytest.raises(zk.ZkError) as e:
        zg.PreparedVk(pp, {"alpha_g1": (1, 2), "beta_g2": None, "gamma_g2": None, "delta_g2": None, "gamma_abc_g1": [(1, 2)]})
    assert e.value.code == 4 and "no pairing parameters" in e.value.msg
