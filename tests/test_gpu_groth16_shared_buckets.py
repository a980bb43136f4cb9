"""The full prover with ONE bucket set for C (csrc/engine_groth16.inc.hpp prove_begin_impl "one bucket set for C"): where the
launches of H, W and U have the same bucket geometry, H runs with r * coef_p as coefficients, H and W donate their buckets
and U's finalize kernel adds them, so that T = r*H + W + U leaves the device as one point.  Every proof below, on a
synthetic R1CS of 2^8 constraints, must reconstruct to the oracle's closed form (A, B, C as multiples of the generators)
and pass zk_groth16_verify:

  * with the five query vectors registered (the shared path: equal 15-bit tables), with zero masks and with all twelve
  * r = 0 (H is not launched: W alone donates) and s = 0
  * only crs.u registered (U has one bucket set, H and W one per window: five reductions as before)
  * table-free (whatever the vectors' lengths give)
  * asynchronously, two proofs in flight
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import groth16 as zg
from zksaas_amd.api import ZK_G1, msm_precompute
from oracle import dist as od
from oracle import groth16 as og
from oracle.curve import g1, g2, GroupOps
from oracle.field import Domain
from oracle.params import BN254
from oracle.prng import rand_fp

from gpu_util import opp, enc_jacobian
from test_oracle_groth16 import small_r1cs

P = BN254.r
NC = 250                         # constraints: a domain of 2^8


@functools.lru_cache(maxsize=None)
def _circuit():
    r1, w = small_r1cs(NC)
    td = [rand_fp(70, i, P) for i in range(5)]
    return r1, w, td, og.setup_scalars(BN254, r1, og.Trapdoor(*td))


class _Prover:
    """a context of its own: the tables it registers do not reach the other tests' contexts"""

    def __init__(self, tables):
        r1, w, td, self.okey = _circuit()
        self.r1, self.w = r1, w
        self.pp = zk.PackedSharingParams("bn254", 2)
        self.setup = zg.SetupScalars("bn254", r1, *td)
        assert self.setup.log_m == 8
        self.crs = zg.Crs(self.pp, self.setup)
        self.wit = zg.Witness(self.pp, "bn254", r1, w, seed=5)
        if tables == "all":
            self.crs.precompute()
        elif tables == "u":
            msm_precompute(self.pp, ZK_G1, self.crs.u, self.pp.n * self.crs.len_u)
        self.pvk = zg.PreparedVk(self.pp, zg.verifying_key(self.pp, self.setup))

    def masks(self):
        pp, setup, o = self.pp, self.setup, opp("bn254", 2)
        m, G1, G2 = setup.m, g1(BN254), g2(BN254)
        keep, mk = [], zg.Masks()
        for k in range(6):
            fmk = zk.FftMask.sample(pp, k < 3, Domain(BN254, 2 * m).element(1) if k < 3 else None, 1 if k < 3 else 0,
                                    setup.log_m, 100 + k)
            keep.append(fmk)
            mk.fft_in[k], mk.fft_out[k] = fmk.in_mask.ptr, fmk.out_mask.ptr
        dm = zk.DegRedMask.sample(pp, m // 2, 200)
        keep.append(dm)
        mk.degred_in, mk.degred_out = dm.in_mask.ptr, dm.out_mask.ptr
        for k in range(5):
            G, is2 = (G2, True) if k == 2 else (G1, False)
            om = od.MsmMask.sample(o, G, GroupOps(G), 300 + k)
            ai = np.stack([enc_jacobian(pp, x.in_mask, is2) for x in om])
            ao = np.stack([enc_jacobian(pp, x.out_mask, is2) for x in om])
            keep += [ai, ao]
            mk.msm_in[k], mk.msm_out[k] = ai.ctypes.data, ao.ctypes.data
        return mk, keep

    def check(self, shares, r, s):
        pp = self.pp
        aff, _ = zg.reconstruct(pp, shares, want_bytes=False)
        v = pp.fq.decode(np.asarray(aff).reshape(-1, pp.fq.nl))
        G1, G2 = g1(BN254), g2(BN254)
        sa, sb, sc_ = og.prove_scalars(BN254, self.r1, self.okey, self.w, r, s)
        assert G1.eq(G1.from_affine((v[0], v[1])), G1.mul(G1.from_affine(BN254.g1), sa))
        assert G2.eq(G2.from_affine(((v[2], v[3]), (v[4], v[5]))), G2.mul(G2.from_affine(BN254.g2), sb))
        assert G1.eq(G1.from_affine((v[6], v[7])), G1.mul(G1.from_affine(BN254.g1), sc_)), "C differs from the oracle"
        assert zg.verify(pp, self.pvk, [aff], [[self.w[1]]]) == [True]

    def close(self):
        self.pvk.free()
        self.pp.close()


@pytest.fixture(scope="module")
def tabled():
    p = _Prover("all")
    yield p
    p.close()


RS = {"plain": (rand_fp(71, 0, P), rand_fp(71, 1, P)), "r_zero": (0, rand_fp(72, 1, P)), "s_zero": (rand_fp(73, 0, P), 0)}


@pytest.mark.parametrize("case", sorted(RS))
def test_shared_bucket_set_zero_masks(tabled, case):
    r, s = RS[case]
    tabled.check(zg.prove(tabled.pp, tabled.crs, tabled.wit, r, s, seed=9), r, s)


@pytest.mark.parametrize("case", ["plain", "r_zero"])
def test_shared_bucket_set_all_twelve_masks(tabled, case):
    r, s = RS[case]
    mk, keep = tabled.masks()
    tabled.check(zg.prove(tabled.pp, tabled.crs, tabled.wit, r, s, masks=mk, seed=11), r, s)
    del keep


def test_shared_bucket_set_checked_prover(tabled):
    r, s = RS["plain"]
    shares, _ = zg.prove(tabled.pp, tabled.crs, tabled.wit, r, s, seed=13, check=True)
    tabled.check(shares, r, s)


def test_two_proofs_in_flight(tabled):
    rs = [(rand_fp(74, 2 * i, P), rand_fp(74, 2 * i + 1, P)) for i in range(4)]
    for i in (0, 2):
        fl = [zg.prove_async(tabled.pp, tabled.crs, tabled.wit, r, s, seed=20 + j) for j, (r, s) in enumerate(rs[i:i + 2])]
        for f, (r, s) in zip(fl, rs[i:i + 2]):
            tabled.check(f.wait(), r, s)


@pytest.mark.parametrize("tables", ["u", "none"])
def test_other_geometries(tables):
    """only U registered: its single bucket set against one set per window of H and W -- nothing is shared; table-free:
    the windows the cost model picks for each vector's length"""
    p = _Prover(tables)
    try:
        for case in ("plain", "r_zero"):
            r, s = RS[case]
            p.check(zg.prove(p.pp, p.crs, p.wit, r, s, seed=9), r, s)
        r, s = RS["plain"]
        mk, keep = p.masks()
        p.check(zg.prove(p.pp, p.crs, p.wit, r, s, masks=mk, seed=11), r, s)
        del keep
    finally:
        p.close()
