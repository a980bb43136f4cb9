"""GPU tests (through the C ABI) for the async and batch forms of the checked prover: zk_groth16_prove_checked_async,
zk_groth16_prove_checked_parties_async, zk_groth16_prove_checked_batch and zk_groth16_prove_checked_batch_async.  The setting
of test_gpu_prove_checked.py, rebuilt here: the small circuit, bn254 at l = 2, all twelve masks; three proofs with distinct
(r, s) and mask seeds.
  honest batch   each proof equals zk_groth16_prove_batch's as group elements per party and reconstructs to the scalars
                 og.verify_scalars accepted; every report is clean
  a liar         party p's rows of qap_a / qap_b / qap_c of proof 1: all three proofs are the honest ones, reports[1] names
                 p in items 0..2, reports[0] and reports[2] are clean; the UNCHECKED batch on the same input gives a proof
                 1 that does not verify and proofs 0 and 2 that do
  async          two checked batches and an unchecked one in flight, waited in reverse order; two checked proofs in flight;
                 a checked proof from n - 1 parties whose id array is overwritten as soon as the call has returned
  no state       the unchecked batch and the unchecked proof after all of that are what they were before"""
import ctypes as C
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
NB, SEED, STEP = 3, 13, 16
LIAR = 5
_state = {}


def _setting():
    """the circuit, its keys, the witness shares, three (r, s) and mask sets, the honest unchecked batch and the input with a
    lying party in proof 1: made once, never changed"""
    if not _state:
        r1, w = small_r1cs()
        pp, o = ctx("bn254", 2), opp("bn254", 2)
        td = [rand_fp(46, i, P) for i in range(5)]
        setup = zg.SetupScalars("bn254", r1, *td)
        okey = og.setup_scalars(BN254, r1, og.Trapdoor(*td))
        crs = zg.Crs(pp, setup)
        wit = zg.Witness(pp, "bn254", r1, w, seed=7)
        masks = [zg.ProofMasks(pp, wit.log_m, 600 + STEP * b) for b in range(NB)]
        rs = [rand_fp(47, 2 * b, P) for b in range(NB)]
        ss = [rand_fp(47, 2 * b + 1, P) for b in range(NB)]
        scalars = [og.prove_scalars(BN254, r1, okey, w, rs[b], ss[b]) for b in range(NB)]
        assert all(og.verify_scalars(BN254, r1, okey, w, sc) for sc in scalars)
        Lc = (1 << wit.log_m) // pp.l
        rng = np.random.default_rng(610)
        qap = []
        for k in range(3):
            rows = wit.qap[k].to_numpy().reshape(pp.n, Lc, 4).copy()
            bad = rng.integers(0, 1 << 63, size=(Lc, 4), dtype=np.uint64)
            bad[:, 3] &= np.uint64((1 << 60) - 1)
            rows[LIAR] = bad
            qap.append(zk.DeviceBuffer.from_numpy(pp, rows))
        lying = types.SimpleNamespace(qap=qap, a_share=wit.a_share, ax_share=wit.ax_share, log_m=wit.log_m, len_a=wit.len_a,
                                      len_w=wit.len_w)
        _state.update(pp=pp, o=o, crs=crs, wit=wit, masks=masks, rs=rs, ss=ss, scalars=scalars, Lc=Lc, lying=lying,
                      honest=zg.prove_batch(pp, crs, [wit] * NB, rs, ss, masks=masks, seed=SEED),
                      single=zg.prove(pp, crs, wit, rs[0], ss[0], masks=masks[0], seed=SEED))
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


def _verifies(S, proof, b):
    """the reconstructed proof is the one og.verify_scalars accepted for (r, s) of proof b (sha256.rs:375-377)"""
    a, b2, c = _points(S.pp, proof)
    o1, o2 = GroupOps(G1), GroupOps(G2)
    sa, sb, sc = S.scalars[b]
    return (G1.eq(S.o.unpack2(a, o1)[0], G1.mul(G1.from_affine(BN254.g1), sa))
            and G2.eq(S.o.unpack2(b2, o2)[0], G2.mul(G2.from_affine(BN254.g2), sb))
            and G1.eq(S.o.unpack2(c, o1)[0], G1.mul(G1.from_affine(BN254.g1), sc)))


def _is_clean(S, rep):
    Lc, pp = S.Lc, S.pp
    return (len(rep.status_host()) == 7 * Lc and not rep.status_host().any() and not rep.errpos_host().any()
            and rep.summaries == [[Lc, 0, 0] + [0] * pp.n] * 7)


def _names(S, rep, p):
    Lc, pp = S.Lc, S.pp
    status, errpos = rep.status_host().reshape(7, Lc), rep.errpos_host().reshape(7, Lc)
    named = [0, Lc, 0] + [Lc if q == p else 0 for q in range(pp.n)]
    return ((status[:3] == 1).all() and (errpos[:3] == 1 << p).all() and not status[3:].any() and not errpos[3:].any()
            and rep.summaries == [named] * 3 + [[Lc, 0, 0] + [0] * pp.n] * 4)


def _lying_batch(S):
    return [S.wit, S.lying, S.wit]


def test_honest_checked_batch_is_the_unchecked_batch():
    S = _setting()
    proofs, reports = zg.prove_batch(S.pp, S.crs, [S.wit] * NB, S.rs, S.ss, masks=S.masks, seed=SEED, check=True)
    assert len(proofs) == NB and len(reports) == NB
    for b in range(NB):
        assert _same_proof(S.pp, proofs[b], S.honest[b]) and _verifies(S, proofs[b], b), b
        assert _is_clean(S, reports[b]), b


def test_a_liar_in_one_proof_is_named_in_its_report_only():
    S = _setting()
    proofs, reports = zg.prove_batch(S.pp, S.crs, _lying_batch(S), S.rs, S.ss, masks=S.masks, seed=SEED, check=True)
    for b in range(NB):
        assert _same_proof(S.pp, proofs[b], S.honest[b]) and _verifies(S, proofs[b], b), b
    assert _names(S, reports[1], LIAR)
    assert _is_clean(S, reports[0]) and _is_clean(S, reports[2])
    # the input bites: the unchecked batch's proof 1 does not verify, its neighbours do
    unchecked = zg.prove_batch(S.pp, S.crs, _lying_batch(S), S.rs, S.ss, masks=S.masks, seed=SEED)
    assert [_verifies(S, unchecked[b], b) for b in range(NB)] == [True, False, True]


def test_checked_and_unchecked_batches_in_flight_together():
    S = _setting()
    pp = S.pp
    f0 = zg.prove_batch_async(pp, S.crs, [S.wit] * NB, S.rs, S.ss, masks=S.masks, seed=SEED, check=True)
    f1 = zg.prove_batch_async(pp, S.crs, _lying_batch(S), S.rs, S.ss, masks=S.masks, seed=SEED, check=True)
    f2 = zg.prove_batch_async(pp, S.crs, [S.wit] * NB, S.rs, S.ss, masks=S.masks, seed=SEED)
    plain = f2.wait()
    lying, lying_reports = f1.wait()
    proofs, reports = f0.wait()
    for b in range(NB):
        assert _same_proof(pp, plain[b], S.honest[b]), b
        assert _same_proof(pp, lying[b], S.honest[b]), b
        assert _same_proof(pp, proofs[b], S.honest[b]), b
        assert _is_clean(S, reports[b]), b
    assert _names(S, lying_reports[1], LIAR) and _is_clean(S, lying_reports[0]) and _is_clean(S, lying_reports[2])


def test_two_checked_proofs_in_flight():
    S = _setting()
    pp = S.pp
    f0 = zg.prove_async(pp, S.crs, S.lying, S.rs[0], S.ss[0], masks=S.masks[0], seed=SEED, check=True)
    f1 = zg.prove_async(pp, S.crs, S.wit, S.rs[1], S.ss[1], masks=S.masks[1], seed=SEED + STEP, check=True)
    p1, r1 = f1.wait()
    p0, r0 = f0.wait()
    assert _same_proof(pp, p0, S.honest[0]) and _verifies(S, p0, 0) and _names(S, r0, LIAR)
    assert _same_proof(pp, p1, S.honest[1]) and _verifies(S, p1, 1) and _is_clean(S, r1)
    # the synchronous call is the asynchronous one followed by the join
    ps, rs_ = zg.prove(pp, S.crs, S.lying, S.rs[0], S.ss[0], masks=S.masks[0], seed=SEED, check=True)
    assert _same_proof(pp, ps, p0) and np.array_equal(rs_.status_host(), r0.status_host())
    assert np.array_equal(rs_.errpos_host(), r0.errpos_host()) and rs_.summaries == r0.summaries


def test_checked_proof_of_a_party_list_owns_its_list():
    S = _setting()
    pp = S.pp
    listed = [q for q in range(pp.n) if q != LIAR]
    want, want_rep = zg.prove(pp, S.crs, S.lying, S.rs[0], S.ss[0], masks=S.masks[0], seed=SEED, check=True, parties=listed)
    ids = (C.c_uint32 * len(listed))(*listed)
    f = zg.prove_async(pp, S.crs, S.lying, S.rs[0], S.ss[0], masks=S.masks[0], seed=SEED, check=True, parties=ids)
    for i in range(len(listed)):                     # the caller's array is the caller's again
        ids[i] = 0xFFFFFFFF
    got, rep = f.wait()
    assert _same_proof(pp, got, want)
    assert np.array_equal(rep.status_host(), want_rep.status_host()) and not rep.status_host().any()
    assert np.array_equal(rep.errpos_host(), want_rep.errpos_host())
    assert rep.summaries == want_rep.summaries and rep.summaries[6] == [0] * (3 + pp.n)      # item 6: not checked with n - 1
    # the liar is the absent party, whose rows are not read: the honest proof
    assert _same_proof(pp, got, S.honest[0]) and _verifies(S, got, 0)


def test_the_checked_forms_leave_no_state():
    S = _setting()
    pp = S.pp
    zg.prove_batch(pp, S.crs, _lying_batch(S), S.rs, S.ss, masks=S.masks, seed=SEED, check=True)
    zg.prove_async(pp, S.crs, S.lying, S.rs[0], S.ss[0], masks=S.masks[0], seed=SEED, check=True).wait()
    again = zg.prove_batch(pp, S.crs, [S.wit] * NB, S.rs, S.ss, masks=S.masks, seed=SEED)
    assert all(_same_proof(pp, again[b], S.honest[b]) for b in range(NB))
    assert _same_proof(pp, zg.prove(pp, S.crs, S.wit, S.rs[0], S.ss[0], masks=S.masks[0], seed=SEED), S.single)
    assert _same_proof(pp, S.single, S.honest[0])
