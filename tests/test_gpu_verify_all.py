"""zk_groth16_verify_all on the device (`pytest -m gpu`): one randomized pairing check for a batch of proofs, against
zk_groth16_verify on the same arrays, the verification equation built from known discrete logarithms, and oracle.pairing for
the value before the comparison.  Everything is an integer: every comparison is exact.

The product of the count + 3 Miller values is split over lane groups by csrc/pairing_rlc_plan.hpp (G = ceil(sqrt(n)) groups
of len = ceil(n / G) values).  No n leaves a group empty; the counts of the discrete-log batches give these shapes:
    count   1   2   5   6   29   30   61   62   300
    n       4   5   8   9   32   33   64   65   303
    G x len 2x2 3x2 3x3 3x3 6x6  6x6  8x8  9x8  18x17
    last    full 1/2 2/3 full 2/6 3/6 full 1/8 14/17      (values in the last group: a partial group wherever it is not full)
and n = 8 | 9, 32 | 33, 64 | 65 are the lane groups of one wave, of one workgroup and of two."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import groth16 as zg
from zksaas_amd.api import ZK_G1, ZK_G2
from oracle import pairing as op
from oracle.curve import g1, g2
from oracle.params import CURVES
from oracle.prng import rand_fp

from gpu_util import ctx
from test_gpu_pairing import _decode_proof, _proofs, flat12

BOTH = ["bn254", "bls12_381"]
NONCE = 0x5A4B524C43
SEED = bytes(range(7, 39))
SEED2 = bytes(range(8, 40))
COUNTS = (1, 2, 5, 6, 29, 30, 61, 62, 300)


def randomizers(seed, count):
    """r_i as the header defines them, from the library's exported block function"""
    lib = zk.load()
    key = (C.c_uint32 * 8)(*struct.unpack("<8I", seed))
    out = (C.c_uint32 * 16)()
    rs = []
    for i in range(count):
        lib.zk_chacha20_block(key, i, NONCE, out)
        rs.append((out[0] | out[1] << 32 | out[2] << 64 | out[3] << 96) or 1)
    return rs


class DlBatch:
    """Key and "proofs" from known discrete logs (the construction of test_verify_with_several_public_inputs): alpha = a G1,
    beta = b G2, gamma = g G2, delta = d G2, abc_t = c_t G1, C_i = cc_i G1, B_i = v_i G2 and A_i = u_i G1 with
    u_i v_i = a b + (c_0 + sum_t x_it c_t) g + cc_i d + err_i (mod r): proof i satisfies the equation iff err_i = 0."""

    def __init__(self, curve, n_inputs, count, tag, xs=None, ident_a=()):
        c = CURVES[curve]
        self.curve, self.c, self.pp, self.r = curve, c, ctx(curve), c.r
        r = c.r
        self.a, self.b, self.g, self.d = (rand_fp(400 + tag, i, r) for i in range(4))
        self.cs = [rand_fp(401 + tag, i, r) for i in range(n_inputs + 1)]
        self.xs = [list(x) for x in xs] if xs is not None else [[rand_fp(402 + tag, i * n_inputs + t, r) for t in range(n_inputs)]
                                                                  for i in range(count)]
        self.count, self.n_inputs = count, n_inputs
        self.cc = [rand_fp(403 + tag, i, r) for i in range(count)]
        self.vv = [rand_fp(404 + tag, i, r) for i in range(count)]
        for i in ident_a:                                  # A = the identity: C chosen so that the equation still holds
            self.cc[i] = -(self.a * self.b + self.lin(i) * self.g) * pow(self.d, -1, r) % r
        pp, nl = self.pp, self.pp.fq.nl
        self.key1 = zg.base_points(pp, ZK_G1, pp.upload_fr([self.a] + self.cs), 1 + len(self.cs)).to_numpy().reshape(-1, 2 * nl)
        self.key2 = zg.base_points(pp, ZK_G2, pp.upload_fr([self.b, self.g, self.d]), 3).to_numpy().reshape(-1, 4 * nl)
        self.vk = {"alpha_g1": self.dec1(self.key1[0]), "gamma_abc_g1": [self.dec1(p) for p in self.key1[1:]],
                   "beta_g2": self.dec2(self.key2[0]), "gamma_g2": self.dec2(self.key2[1]), "delta_g2": self.dec2(self.key2[2])}
        self.pvk = zg.PreparedVk(pp, self.vk)
        self.good = self.proofs()

    def dec1(self, row):
        v = tuple(self.pp.fq.decode(np.asarray(row).reshape(2, self.pp.fq.nl)))
        return None if v == (0, 0) else v

    def dec2(self, row):
        v = self.pp.fq.decode(np.asarray(row).reshape(4, self.pp.fq.nl))
        return ((v[0], v[1]), (v[2], v[3]))

    def lin(self, i, xs=None):
        x = (xs or self.xs)[i]
        return (self.cs[0] + sum(v * k for v, k in zip(x, self.cs[1:]))) % self.r

    def proofs(self, err=None):
        """[count][8 nl] rows A | B | C; err: {proof: err_i}"""
        pp, nl, r, n = self.pp, self.pp.fq.nl, self.r, self.count
        err = err or {}
        uu = [(self.a * self.b + self.lin(i) * self.g + self.cc[i] * self.d + err.get(i, 0)) * pow(self.vv[i], -1, r) % r
              for i in range(n)]
        p1 = zg.base_points(pp, ZK_G1, pp.upload_fr(uu + self.cc[:n]), 2 * n).to_numpy().reshape(-1, 2 * nl)
        if not hasattr(self, "_b"):
            self._b = zg.base_points(pp, ZK_G2, pp.upload_fr(self.vv), n).to_numpy().reshape(-1, 4 * nl)
        return np.ascontiguousarray(np.concatenate([p1[:n], self._b, p1[n:]], axis=1))


EDGE_XS = lambda r: [[0, 1, r - 1, rand_fp(332, 0, r)], [(1 << 64) - 1, ((1 << 128) - 1) << 64, r - 2, 2], [0, 0, 0, 0]]


@functools.lru_cache(maxsize=None)
def _dl300(curve):
    r = CURVES[curve].r
    xs = EDGE_XS(r) + [[rand_fp(410, 4 * i + t, r) for t in range(4)] for i in range(3, 300)]
    xs[299] = [r - 1, 0, (1 << 64) - 1, 1]                  # the edge values also in the last proof
    return DlBatch(curve, 4, 300, 0, xs)


def both(pp, pvk, proofs, xs, seed=SEED):
    """(verify_all, verify) on the same arrays"""
    return zg.verify_all(pp, pvk, proofs, xs, seed=seed), zg.verify(pp, pvk, proofs, xs)


# ------------------------------------------------------------------------------------------------------ 1, 2, 3: real proofs
@pytest.mark.parametrize("curve", BOTH)
def test_real_proofs_are_accepted_also_alone_and_from_a_party_subset(curve):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    assert zg.verify_all(pp, pvk, affs, [[w[1]]] * 5, seed=SEED) is True
    assert zg.verify_all(pp, pvk, [affs[0]], [[w[1]]], seed=SEED) is True
    present = [0, 1, 2, 4, 5, 6, 7]
    sub, _ = zg.reconstruct(pp, tuple(x[present] for x in shares[1]), parties=present, want_bytes=False)
    assert zg.verify_all(pp, pvk, [sub], [[w[1]]], seed=SEED) is True


@pytest.mark.parametrize("curve", BOTH)
def test_swapped_c_is_rejected(curve):
    """sum C_i and prod e(A_i, B_i) are unchanged by the swap: a sum without randomizers (or with repeated ones) accepts it"""
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    nl = pp.fq.nl
    batch = [a.copy() for a in affs]
    batch[1][6 * nl:], batch[3][6 * nl:] = affs[3][6 * nl:], affs[1][6 * nl:]
    assert both(pp, pvk, batch, [[w[1]]] * 5) == (False, [True, False, True, False, True])
    assert zg.verify_all(pp, pvk, batch, [[w[1]]] * 5, seed=SEED2) is False


def _raw_add_q(pp, c, limbs):
    """the same residue written as a value >= q (little-endian 64-bit limbs)"""
    v = sum(int(x) << (64 * j) for j, x in enumerate(limbs)) + c.q
    assert v < 1 << (64 * pp.fq.nl)
    return np.array([(v >> (64 * j)) & ((1 << 64) - 1) for j in range(pp.fq.nl)], dtype=np.uint64)


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("defect", ["input", "replaced_a", "a_y", "b_y_c1", "c_y", "not_canonical"])
def test_one_defect_at_the_first_a_middle_and_the_last_position(curve, defect):
    pp, c, w, vk, pvk, shares, affs = _proofs(curve)
    nl = pp.fq.nl
    for pos in (0, 2, 4):
        batch, xs = [a.copy() for a in affs], [[w[1]] for _ in range(5)]
        if defect == "input":
            xs[pos] = [(w[1] + 1) % c.r]
        elif defect == "replaced_a":
            batch[pos][:2 * nl] = affs[(pos + 1) % 5][:2 * nl]
        elif defect == "not_canonical":
            batch[pos][6 * nl:7 * nl] = _raw_add_q(pp, c, batch[pos][6 * nl:7 * nl])          # x of C
        else:
            lo = {"a_y": nl, "b_y_c1": 5 * nl, "c_y": 7 * nl}[defect]
            v = pp.fq.decode(batch[pos][lo:lo + nl])[0]
            batch[pos][lo:lo + nl] = pp.fq.encode_one((v + 1) % c.q)
        assert both(pp, pvk, batch, xs) == (False, [j != pos for j in range(5)]), (defect, pos)


# ------------------------------------------------------------------------------------------- 4: discrete-log batches
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("count", COUNTS)
def test_discrete_log_batches_at_the_fold_shapes(curve, count):
    """True for the batch; False with one error in the last proof, and in proof count // 2 (see the table in the docstring
    of this file for the shape each count gives the product)."""
    d = _dl300(curve)
    pp = d.pp
    pr, xs = d.good[:count], d.xs[:count]
    assert zg.verify_all(pp, d.pvk, pr, xs, seed=SEED) is True
    for pos in {count - 1, count // 2}:
        bad = [list(x) for x in xs]
        bad[pos][pos % 4] = (bad[pos][pos % 4] + 1) % d.r
        assert zg.verify_all(pp, d.pvk, pr, bad, seed=SEED) is False, pos


# --------------------------------------------------------------------------------- 5: the derivation through the mathematics
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("count", [3, 62])
def test_errors_that_cancel_under_the_seeds_randomizers(curve, count):
    """Errors e_i != 0 with sum r_i e_i = 0 (mod r) for the r_i of SEED: the batch check with SEED accepts what every
    per-proof check rejects, with another seed it rejects.  That needs the counter, the nonce, the word order and the Fr sums
    to be exactly the documented ones.  count 62: n = 65 Miller values in 9 groups of 8; proofs 3, 20, 41 and 61 fall in
    groups 0, 2, 5 and 7."""
    d = _dl300(curve)
    pp, r = d.pp, d.r
    touched = [0, 1, 2] if count == 3 else [3, 20, 41, 61]
    rs = randomizers(SEED, count)
    err = {i: rand_fp(420, i, r) or 1 for i in touched[:-1]}
    last = touched[-1]
    err[last] = -sum(rs[i] * e for i, e in err.items()) * pow(rs[last], -1, r) % r
    assert all(err.values()) and sum(rs[i] * e for i, e in err.items()) % r == 0
    sub = DlBatch.__new__(DlBatch)
    sub.__dict__.update(d.__dict__)
    sub.count, sub._b = count, d._b[:count]
    pr, xs = sub.proofs(err), d.xs[:count]
    assert zg.verify_all(pp, d.pvk, pr, xs, seed=SEED) is True
    assert zg.verify_all(pp, d.pvk, pr, xs, seed=SEED2) is False
    assert zg.verify(pp, d.pvk, pr, xs) == [i not in err for i in range(count)]


# ------------------------------------------------------------------------------------------------ 6: gt_out against the oracle
@pytest.mark.parametrize("curve", BOTH)
def test_gt_out_equals_the_oracles_product_of_the_five_pairs(curve):
    c = CURVES[curve]
    d = DlBatch(curve, 2, 2, 10)
    pp, r = d.pp, d.r
    G1, G2, pr = g1(c), g2(c), op.pairing_for(c)
    one = [1] + [0] * 11
    ok, gt = zg.verify_all(pp, d.pvk, d.good, d.xs, seed=SEED, want_gt=True)
    assert ok is True and gt == one
    bad = d.proofs({1: 5})
    ok, gt = zg.verify_all(pp, d.pvk, bad, d.xs, seed=SEED, want_gt=True)
    assert ok is False
    rs = randomizers(SEED, 2)
    mul1 = lambda p, k: G1.to_affine(G1.mul(G1.from_affine(p), k % r))
    neg2 = lambda q: G2.to_affine(G2.neg(G2.from_affine(q)))
    proofs = [_decode_proof(pp, row) for row in bad]
    s = sum(rs) % r
    st = [sum(ri * x[t] for ri, x in zip(rs, d.xs)) % r for t in range(2)]
    abc = d.vk["gamma_abc_g1"]
    pg = G1.mul(G1.from_affine(abc[0]), s)
    for t in range(2):
        pg = G1.add(pg, G1.mul(G1.from_affine(abc[t + 1]), st[t]))
    pd = G1.add(G1.mul(G1.from_affine(proofs[0][2]), rs[0]), G1.mul(G1.from_affine(proofs[1][2]), rs[1]))
    pairs = [(mul1(A, ri), B) for (A, B, _), ri in zip(proofs, rs)]
    pairs += [(G1.to_affine(pg), neg2(d.vk["gamma_g2"])), (G1.to_affine(pd), neg2(d.vk["delta_g2"])),
              (mul1(d.vk["alpha_g1"], -s), d.vk["beta_g2"])]
    want = flat12(pr.multi_pairing(pairs))
    assert want != one and gt == want


# ---------------------------------------------------------------------------------------------------------------- 7: corners
@pytest.mark.parametrize("curve", BOTH)
def test_corners_no_inputs_identity_a_empty_batch_drawn_seed(curve):
    d0 = DlBatch(curve, 0, 3, 20)                            # n_abc = 1
    assert both(d0.pp, d0.pvk, d0.good, d0.xs) == (True, [True] * 3)
    assert zg.verify_all(d0.pp, d0.pvk, d0.proofs({1: 1}), d0.xs, seed=SEED) is False
    di = DlBatch(curve, 2, 3, 21, ident_a=(1,))              # A of proof 1 = the identity, the equation still holds
    nl = di.pp.fq.nl
    assert not di.good[1][:2 * nl].any() and di.good[0][:2 * nl].any()
    assert both(di.pp, di.pvk, di.good, di.xs) == (True, [True] * 3)
    d = _dl300(curve)
    pp = d.pp
    assert zg.verify_all(pp, d.pvk, np.zeros((0, 8 * nl), dtype=np.uint64), []) is True
    assert zg.verify_all(pp, d.pvk, np.zeros((0, 8 * nl), dtype=np.uint64), [], want_gt=True) == (True, [1] + [0] * 11)
    bad = [list(x) for x in d.xs[:6]]
    bad[4][0] += 1
    for _ in range(2):                                       # seed = None: the library draws one
        assert zg.verify_all(pp, d.pvk, d.good[:6], d.xs[:6]) is True
        assert zg.verify_all(pp, d.pvk, d.good[:6], bad) is False


@pytest.mark.parametrize("curve", BOTH)
def test_a_key_with_twenty_inputs_takes_more_than_one_wave_of_the_gamma_fold(curve):
    """21 key points: three waves of eight rows in pairing_rlc_gamma_kernel, their partial sums folded"""
    d = DlBatch(curve, 20, 3, 30)
    assert both(d.pp, d.pvk, d.good, d.xs) == (True, [True] * 3)
    bad = [list(x) for x in d.xs]
    bad[2][19] = (bad[2][19] + 1) % d.r
    assert both(d.pp, d.pvk, d.good, bad) == (False, [True, True, False])


# ------------------------------------------------------------------------------------------------- 8, 9: agreement, workspace
@pytest.mark.parametrize("curve", BOTH)
def test_agreement_with_the_per_proof_verifier_on_33_proofs(curve):
    d = _dl300(curve)
    pp, xs = d.pp, d.xs[:33]
    for nbad, where in ((0, []), (1, [17]), (2, [0, 32]), (33, list(range(33)))):
        sub = DlBatch.__new__(DlBatch)
        sub.__dict__.update(d.__dict__)
        sub.count, sub._b = 33, d._b[:33]
        pr = sub.proofs({i: i + 1 for i in where})
        each = zg.verify(pp, d.pvk, pr, xs)
        assert each == [i not in where for i in range(33)]
        assert zg.verify_all(pp, d.pvk, pr, xs, seed=SEED) == all(each), nbad


@pytest.mark.parametrize("curve", BOTH)
def test_the_two_calls_share_one_workspace(curve):
    """verify (300), verify_all (300), verify_all (1), verify (5) on one context: what each gives alone"""
    d = _dl300(curve)
    pp = d.pp
    bad = [list(x) for x in d.xs]
    bad[123][2] = (bad[123][2] + 1) % d.r
    assert zg.verify(pp, d.pvk, d.good, bad) == [i != 123 for i in range(300)]
    assert zg.verify_all(pp, d.pvk, d.good, bad, seed=SEED) is False
    assert zg.verify_all(pp, d.pvk, d.good[:1], d.xs[:1], seed=SEED) is True
    assert zg.verify(pp, d.pvk, d.good[:5], bad[:5]) == [True] * 5
    assert zg.verify_all(pp, d.pvk, d.good, d.xs, seed=SEED) is True


# ----------------------------------------------------------------------------------------------------------------- 10: errors
def test_argument_errors_are_those_of_the_per_proof_call():
    d = _dl300("bn254")
    pp = d.pp
    for xs in ([1, 2, 3], [1, 2, 3, 4, 5]):
        with pytest.raises(zk.ZkError) as e:
            zg.verify_all(pp, d.pvk, d.good[:1], [xs])
        assert e.value.code == 4 and "malformed verifying key" in e.value.msg
    p377 = ctx("bls12_377")
    with pytest.raises(zk.ZkError) as e:
        zg.verify_all(p377, type("V", (), {"h": None, "n_abc": 2})(), [np.zeros(8 * p377.fq.nl, dtype=np.uint64)], [[1]])
    assert e.value.code == 4 and "no pairing parameters" in e.value.msg
    other = ctx("bls12_381")                                 # a key of another context
    with pytest.raises(zk.ZkError) as e:
        zg.verify_all(other, d.pvk, [np.zeros(8 * other.fq.nl, dtype=np.uint64)], [[1, 2, 3, 4]])
    assert e.value.code == 4 and "another context" in e.value.msg
