"""GPU tests (through the C ABI) for zk_groth16_prove_checked: zk_groth16_prove with h computed by the checked chain of
zk_circom_h_checked on the prover's own stream and work buffers.  The small circuit of test_gpu_groth16.py, all twelve masks,
bn254 at l = 2.
  honest input   the proof equals zk_groth16_prove's as group elements per party and verifies; the report is all clean
  a lying party  its rows of qap_a / qap_b / qap_c replaced: the checked proof is the honest proof and verifies, items 0..2
                 name the party in every chunk; the unchecked prover's proof on the same input does not verify
  no state       an unchecked proof after a checked one on the same context is the proof it was before"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import groth16 as zg
from oracle import groth16 as og
from oracle.curve import g1, g2, GroupOps
from oracle.params import BN254
from oracle.prng import rand_fp

from gpu_util import ctx, opp, dec_jacobian
from test_oracle_groth16 import small_r1cs

P = BN254.r
G1, G2 = g1(BN254), g2(BN254)
_state = {}


def _setting():
    """the circuit, its keys, the witness shares, the masks and the honest unchecked proof: made once, never changed"""
    if not _state:
        r1, w = small_r1cs()
        pp, o = ctx("bn254", 2), opp("bn254", 2)
        td = [rand_fp(46, i, P) for i in range(5)]
        setup = zg.SetupScalars("bn254", r1, *td)
        okey = og.setup_scalars(BN254, r1, og.Trapdoor(*td))
        crs = zg.Crs(pp, setup)
        wit = zg.Witness(pp, "bn254", r1, w, seed=7)
        masks = zg.ProofMasks(pp, wit.log_m, 600)
        r, s = rand_fp(47, 0, P), rand_fp(47, 1, P)
        scalars = og.prove_scalars(BN254, r1, okey, w, r, s)
        assert og.verify_scalars(BN254, r1, okey, w, scalars)
        _state.update(pp=pp, o=o, crs=crs, wit=wit, masks=masks, r=r, s=s, scalars=scalars,
                      honest=zg.prove(pp, crs, wit, r, s, masks=masks, seed=13))
    return types.SimpleNamespace(**_state)


def _points(pp, proof):
    pa, pb, pc = proof
    return ([dec_jacobian(pp, pa[i]) for i in range(pp.n)], [dec_jacobian(pp, pb[i], True) for i in range(pp.n)],
            [dec_jacobian(pp, pc[i]) for i in range(pp.n)])


def _same_proof(pp, x, y):
    """equal as group elements per party (the MSM's Jacobian bytes are not canonical)"""
    (xa, xb, xc), (ya, yb, yc) = _points(pp, x), _points(pp, y)
    return (all(G1.eq(u, v) for u, v in zip(xa, ya)) and all(G2.eq(u, v) for u, v in zip(xb, yb))
            and all(G1.eq(u, v) for u, v in zip(xc, yc)))


def _verifies(S, proof):
    """the reconstructed proof is the one og.verify_scalars accepted (sha256.rs:375-377)"""
    a, b, c = _points(S.pp, proof)
    o1, o2 = GroupOps(G1), GroupOps(G2)
    sa, sb, sc = S.scalars
    return (G1.eq(S.o.unpack2(a, o1)[0], G1.mul(G1.from_affine(BN254.g1), sa))
            and G2.eq(S.o.unpack2(b, o2)[0], G2.mul(G2.from_affine(BN254.g2), sb))
            and G1.eq(S.o.unpack2(c, o1)[0], G1.mul(G1.from_affine(BN254.g1), sc)))


def _clean(pp, Lc):
    return [Lc, 0, 0] + [0] * pp.n


def test_honest_checked_proof_equals_the_unchecked_one_and_leaves_no_state():
    S = _setting()
    pp, Lc = S.pp, (1 << S.wit.log_m) // S.pp.l
    assert _verifies(S, S.honest)
    proof, rep = zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13, check=True)
    assert _same_proof(pp, proof, S.honest) and _verifies(S, proof)
    assert not rep.status_host().any() and not rep.errpos_host().any() and len(rep.status_host()) == 7 * Lc
    assert rep.summaries == [_clean(pp, Lc)] * 7
    # the optional report leaves nothing behind: the unchecked prover gives the proof it gave before
    again = zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13)
    assert _same_proof(pp, again, S.honest)


def test_a_lying_party_is_named_and_the_proof_is_the_honest_one():
    S = _setting()
    pp, Lc = S.pp, (1 << S.wit.log_m) // S.pp.l
    p = 5
    rng = np.random.default_rng(610)
    qap = []
    for k in range(3):
        rows = S.wit.qap[k].to_numpy().reshape(pp.n, Lc, 4).copy()
        bad = rng.integers(0, 1 << 63, size=(Lc, 4), dtype=np.uint64)
        bad[:, 3] &= np.uint64((1 << 60) - 1)
        rows[p] = bad
        qap.append(zk.DeviceBuffer.from_numpy(pp, rows))
    wit = types.SimpleNamespace(qap=qap, a_share=S.wit.a_share, ax_share=S.wit.ax_share, log_m=S.wit.log_m,
                                len_a=S.wit.len_a, len_w=S.wit.len_w)
    proof, rep = zg.prove(pp, S.crs, wit, S.r, S.s, masks=S.masks, seed=13, check=True)
    assert _same_proof(pp, proof, S.honest) and _verifies(S, proof)
    status, errpos = rep.status_host().reshape(7, Lc), rep.errpos_host().reshape(7, Lc)
    assert (status[:3] == 1).all() and (errpos[:3] == 1 << p).all() and not status[3:].any() and not errpos[3:].any()
    named = [0, Lc, 0] + [Lc if q == p else 0 for q in range(pp.n)]
    assert rep.summaries == [named] * 3 + [_clean(pp, Lc)] * 4
    # the input bites: the unchecked prover's proof on it does not verify
    assert not _verifies(S, zg.prove(pp, S.crs, wit, S.r, S.s, masks=S.masks, seed=13))
    # and the context is as it was
    assert _same_proof(pp, zg.prove(pp, S.crs, S.wit, S.r, S.s, masks=S.masks, seed=13), S.honest)
