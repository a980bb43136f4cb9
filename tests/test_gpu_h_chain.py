"""GPU tests that tie the one h chain (csrc/engine_h.inc.hpp h_chain) to the Python oracle.  The other circom_h tests compare
the forms of the chain with each other, and every form is the same driver; these compare with oracle/groth16.py circom_h:
  batch           zk_circom_h_batch_checked, nb = 2: h of each proof, share for share, is the oracle's with seed + 16 b
  partial masks   zk_circom_h_checked with the in-masks of items 1, 3 and 4 absent (a null in-mask is the oracle's in-mask
                  of zeros; the out-mask stays): the word step scales and adds per item, the kings run item by item
bn254, l = 2, m = 64 as test_gpu_circom_h_checked.py test_honest_h_equals_the_oracle (ext_wit.rs:419-538: a = b = [0..m),
c = a*b, masked); the second proof of the batch has a second input of the same shape.  Each input's oracle h is computed once."""
import pytest

pytestmark = pytest.mark.gpu

from zksaas_amd import api
from zksaas_amd import groth16 as zg
from oracle import dist as od
from oracle import groth16 as og
from oracle.field import Domain
from oracle.params import BN254

from gpu_util import ctx, opp, up_parties, down_parties

M, L, LOG_M = 64, 2, 6
SEED, STEP = 4, 16             # PROOF_SEED_STEP
PARTIAL = (1, 3, 4)            # the "partial" set of test_gpu_circom_h_checked.py: round 1 a and c masked, round 2 c only

_cases = {}


def _case(b, partial):
    """(device QAP vectors, zk_groth16_masks, the oracle's h with seed + 16 b, what keeps the buffers alive) of input b"""
    key = (b, partial)
    if key in _cases:
        return _cases[key]
    pp, o = ctx("bn254", L), opp("bn254", L)
    P = BN254.r
    dom = Domain(BN254, M)
    a = list(range(M)) if b == 0 else [(7 * i + 3) % P for i in range(M)]
    bb = a if b == 0 else [(M - i) * (M - i) % P for i in range(M)]
    c = [x * y % P for x, y in zip(a, bb)]
    qs = og.QAP(0, 0, a, bb, c, dom).pss(o, 3 + 10 * b)
    w2m = Domain(BN254, 2 * M).element(1)
    fm = ([od.FftMask.sample(True, w2m, dom.group_gen_inv, M, o, 40 + 100 * b + k) for k in range(3)]
          + [od.FftMask.sample(False, 1, dom.group_gen, M, o, 50 + 100 * b + k) for k in range(3)])
    dm = od.DegRedMask.sample(o, 1, M // L, 60 + 100 * b)
    if partial:
        for k in PARTIAL:
            fm[k] = [od.FftMask([0] * (M // L), x.out_mask) for x in fm[k]]
    want = og.circom_h(qs, fm, dm, o, dom, seed=SEED + STEP * b)
    bufs = [up_parties(pp, [qs[i][k] for i in range(o.n)]) for k in range(3)]
    keep = []
    mk = zg.Masks()
    for k in range(6):
        bo = up_parties(pp, [x.out_mask for x in fm[k]])
        keep.append(bo)
        mk.fft_out[k] = bo.ptr
        if not (partial and k in PARTIAL):
            bi = up_parties(pp, [x.in_mask for x in fm[k]])
            keep.append(bi)
            mk.fft_in[k] = bi.ptr
    di, do = up_parties(pp, [x.in_mask for x in dm]), up_parties(pp, [x.out_mask for x in dm])
    keep += [di, do]
    mk.degred_in, mk.degred_out = di.ptr, do.ptr
    _cases[key] = (bufs, mk, want, keep)
    return _cases[key]


def _clean(pp, rep):
    return not rep.status_host().any() and rep.summaries == [[M // L] + [0] * (2 + pp.n)] * 7


@pytest.mark.parametrize("partial", [False, True], ids=["all", "partial"])
def test_batch_of_two_equals_the_oracle(partial):
    pp = ctx("bn254", L)
    cases = [_case(b, partial) for b in range(2)]
    hs, reps = api.circom_h_batch_checked(pp, [c[0] for c in cases], [c[1] for c in cases], SEED, log2_m=LOG_M)
    for b in range(2):
        assert down_parties(pp, hs[b], pp.n, M // L) == cases[b][2], (b, partial)
        assert _clean(pp, reps[b]), (b, partial)


def test_single_checked_call_with_partial_masks_equals_the_oracle():
    pp = ctx("bn254", L)
    bufs, mk, want, _ = _case(0, True)
    h, rep = api.circom_h(pp, bufs, mk, SEED, check=True, log2_m=LOG_M)
    assert down_parties(pp, h, pp.n, M // L) == want
    assert _clean(pp, rep)
    # and the unchecked chain, whose kings take the in-masks themselves
    assert down_parties(pp, api.circom_h(pp, bufs, mk, SEED, log2_m=LOG_M), pp.n, M // L) == want
