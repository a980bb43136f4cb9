"""-m gpu: the batched dealer -- zk_base_mul_few (a lane group per scalar), zk_groth16_deal_masks (the twelve masks of
nproofs proofs in one call) and zk_groth16_deal_witness (device witness -> the prover's five share vectors) -- against
the oracle and against the single calls they replace.

A note on the "opposite partial sums" case of zk_base_mul_few.  The kernel works on the CANONICAL scalar x < r and the
partial sums of its tree are s_A * Base for sums s_A of disjoint digit subsets of x, so 0 <= s_A + s_B <= x < r: with a
base of order r (every generator) two tree inputs are never equal or opposite unless both are the identity.  The adder
of the tree handles those cases all the same; to reach them through the public interface the test multiplies a base of
order THREE, (0, 2) on y^2 = x^3 + 4 (BLS12-381) and (0, 1) on y^2 = x^3 + 1 (BLS12-377): 256 = 1 mod 3, so the table
entry of digit d in any window is (d mod 3) * T, and digits 1 | 1 meet as T + T, digits 1 | 2 as T + (-T).  Digits that
are multiples of 3 are kept out (their table entries are the identity, which the table cannot hold).  The scalars x and
r - x of a generator are checked as well: their products are opposite points."""
import ctypes as C
import functools

import numpy as np
import pytest

import zksaas_amd as zk
from oracle import dist as od
from oracle import groth16 as og
from oracle.curve import GroupOps, g1, g2
from oracle.params import BN254, CURVES
from oracle.prng import rand_fp, rand_vec
from zksaas_amd import circom
from zksaas_amd import groth16 as zg
from zksaas_amd import sha256_circuit as sc
from zksaas_amd.api import ZK_G1, ZK_G2

from gpu_util import ctx, dec_jacobian, enc_affine, opp
from test_oracle_groth16 import small_r1cs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ zk_base_mul_few
def _few(pp, group, base_row, scalars):
    is2 = group == ZK_G2
    nl = pp.fq.nl * (2 if is2 else 1)
    out = zk.api.base_mul_few(pp, group, base_row, pp.upload_fr(scalars), len(scalars))
    pp.sync()
    rows = out.to_numpy().reshape(-1, 3 * nl)[:len(scalars)]
    return [dec_jacobian(pp, rows[i], is2) for i in range(len(scalars))]


def _edge_scalars(r):
    nwin = (r.bit_length() + 7) // 8
    top = r >> (8 * (nwin - 1))                                  # the top window's largest digit
    x = rand_fp(71, 0, r)
    edge = [0, 1, 2, r - 1, 255, 256, 1 << (8 * 13), 1 << (8 * (nwin - 1)),
            ((top - 1) << (8 * (nwin - 1))) | ((1 << (8 * (nwin - 1))) - 1),      # digit 255 in every window below the top
            0xAB << (8 * 17),                                                     # a single non-zero window
            x, r - x]                                                             # opposite products
    return edge + [0xFFFF << (8 * 7)], x                                          # two full digits in the lanes 7 and 0


@pytest.mark.parametrize("curve,group", [("bn254", ZK_G1), ("bn254", ZK_G2), ("bls12_381", ZK_G1), ("bls12_377", ZK_G1)])
def test_base_mul_few_matches_the_oracle(curve, group):
    pp, c = ctx(curve, 2), CURVES[curve]
    is2 = group == ZK_G2
    G = g2(c) if is2 else g1(c)
    gen = G.from_affine(G.gen)
    edge, x = _edge_scalars(c.r)
    scalars = edge + rand_vec(72, 24, c.r)
    assert len(scalars) == 37                                    # 37 * 8 lanes: the last workgroup is partly filled
    got = _few(pp, group, enc_affine(pp, [G.gen], is2)[0], scalars)
    for s, p in zip(scalars, got):
        assert G.eq(p, G.mul(gen, s)), hex(s)
    assert got[0][2] in (0, (0, 0))                              # the zero scalar: Jacobian identity, Z = 0
    ix = scalars.index(x)
    assert G.eq(G.add(got[ix], got[ix + 1]), G.mul(gen, 0))      # x G + (r - x) G


def test_base_mul_few_empty_and_over_the_bound():
    pp = ctx("bn254", 2)
    G = g1(BN254)
    base = enc_affine(pp, [G.gen])[0]
    zk.api.base_mul_few(pp, ZK_G1, base, None, 0)                # len = 0: OK, nothing is read
    n = zk.api.BASE_MUL_FEW_MAX + 1
    with pytest.raises(zk.ZkError) as e:
        zk.api.base_mul_few(pp, ZK_G1, base, pp.alloc_fr(n), n)
    assert "zk_base_mul" in str(e.value)
    with pytest.raises(zk.ZkError):
        zk.api.base_mul_few(ctx("bls12_377", 2), ZK_G2, np.zeros(4 * 6, dtype=np.uint64), pp.alloc_fr(1), 1)


@pytest.mark.parametrize("curve,point", [("bls12_381", (0, 2)), ("bls12_377", (0, 1))])
def test_base_mul_few_tree_adds_equal_and_opposite_partial_sums(curve, point):
    """A base of order 3 (module docstring): tree inputs that are equal (doubling), opposite (identity) and identities."""
    pp, c = ctx(curve, 2), CURVES[curve]
    G = g1(c)
    T = G.from_affine(point)
    assert (point[1] ** 2 - point[0] ** 3) % c.q in (1, 4) and G.eq(G.mul(T, 3), G.mul(T, 0))
    d = lambda *pairs: sum(v << (8 * w) for w, v in pairs)
    scalars = [d((0, 1), (1, 1)),                       # level 0: T + T
               d((0, 1), (1, 2)),                       # level 0: T + 2T = identity
               d((0, 2), (2, 1)),                       # level 1: 2T + T
               d((0, 1), (1, 1), (2, 1), (3, 1)),       # level 0: two doublings, level 1: 2T + 2T
               d((0, 1), (4, 1)),                       # level 2: T + T
               d((0, 1), (1, 1), (4, 2), (5, 2)),       # level 2: 2T + 4T = 2T + T
               d((0, 1), (8, 1)),                       # inside one lane: the mixed addition meets its own point
               d((0, 1), (8, 2)),                       # ... and its negative
               d(*[(w, 1 + (w % 2)) for w in range(31)]),
               d(*[(w, 1) for w in range(31)])]
    got = _few(pp, ZK_G1, enc_affine(pp, [point])[0], scalars)
    for s, p in zip(scalars, got):
        assert G.eq(p, G.mul(T, s % 3)), hex(s)


# ------------------------------------------------------------------------------------------------ zk_groth16_deal_masks
def _gens(pp, curve):
    c = CURVES[curve]
    return enc_affine(pp, [g1(c).gen])[0], enc_affine(pp, [g2(c).gen], True)[0]


@functools.lru_cache(maxsize=None)
def _oracle_msm_mask(curve, l, is2, seed):
    c, o = CURVES[curve], opp(curve, l)
    G = g2(c) if is2 else g1(c)
    return od.MsmMask.sample(o, G, GroupOps(G), seed)


def _assert_masks_equal_single_calls(pp, curve, log_m, seed, dealt):
    """dealt: ProofMasks-like objects (.fft, .degred, .msm), proof b against the single samplers at seed + 16 b."""
    c, o = CURVES[curve], opp(curve, pp.l)
    g1row, g2row = _gens(pp, curve)
    w2m = zg._root_of_unity(curve, log_m + 1)
    for b, pm in enumerate(dealt):
        sb = seed + 16 * b
        for k in range(6):
            want = zk.FftMask.sample(pp, k < 3, w2m if k < 3 else None, 1 if k < 3 else 0, log_m, sb + k)
            assert np.array_equal(pm.fft[k].in_mask.to_numpy(), want.in_mask.to_numpy()), (b, k)
            assert np.array_equal(pm.fft[k].out_mask.to_numpy(), want.out_mask.to_numpy()), (b, k)
        want = zk.DegRedMask.sample(pp, (1 << log_m) // pp.l, sb + 6)
        assert np.array_equal(pm.degred.in_mask.to_numpy(), want.in_mask.to_numpy()), b
        assert np.array_equal(pm.degred.out_mask.to_numpy(), want.out_mask.to_numpy()), b
        for k in range(5):
            is2 = k == 2
            G = g2(c) if is2 else g1(c)
            ops = GroupOps(G)
            single = zk.MsmMask.sample(pp, ZK_G2 if is2 else ZK_G1, g2row if is2 else g1row, sb + 7 + k)
            orc = _oracle_msm_mask(curve, pp.l, is2, sb + 7 + k)
            ins = [dec_jacobian(pp, pm.msm[k].in_mask[i], is2) for i in range(pp.n)]
            outs = [dec_jacobian(pp, pm.msm[k].out_mask[i], is2) for i in range(pp.n)]
            for i in range(pp.n):
                assert G.eq(ins[i], dec_jacobian(pp, single.in_mask[i], is2)), (b, k, i)
                assert G.eq(outs[i], dec_jacobian(pp, single.out_mask[i], is2)), (b, k, i)
                assert G.eq(ins[i], orc[i].in_mask) and G.eq(outs[i], orc[i].out_mask), (b, k, i)
            # dmsm/mod.rs:34: the out-mask secrets are all minus the sum of the in-mask secrets
            si, so = o.unpack(ins, ops), o.unpack(outs, ops)
            assert G.eq(G.neg(G.sum(si)), so[0]) and all(G.eq(so[0], x) for x in so[1:]), (b, k)


@pytest.mark.parametrize("l,log_m,nproofs", [(2, 1, 1), (2, 5, 1), (2, 5, 3), (4, 4, 2)])
def test_deal_masks_equals_the_single_calls(l, log_m, nproofs):
    pp = ctx("bn254", l)
    dealt = zg.ProofMasks.batch(pp, log_m, 1000, nproofs)
    pp.sync()
    _assert_masks_equal_single_calls(pp, "bn254", log_m, 1000, dealt)
    if nproofs == 1:                                             # ProofMasks itself is the nproofs = 1 call
        one = zg.ProofMasks(pp, log_m, 1000)
        pp.sync()
        _assert_masks_equal_single_calls(pp, "bn254", log_m, 1000, [one])


def test_deal_masks_leaves_skipped_slots_alone_and_rejects_a_missing_g2():
    pp = ctx("bn254", 2)
    log_m = 3
    g1row, g2row = _gens(pp, "bn254")
    pm = zg.ProofMasks.__new__(zg.ProofMasks)
    pm._alloc(pp, log_m)
    fill = np.full(pm.fft[1].in_mask.nbytes // 8, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    for buf in (pm.fft[1].in_mask, pm.fft[1].out_mask, pm.degred.in_mask, pm.degred.out_mask):
        pp._check(pp.lib.zk_memcpy_h2d(pp.h, buf.ptr, fill.ctypes.data, fill.nbytes, None))
    for k in (2, 3):
        pm.msm[k].in_mask[:] = 7
        pm.msm[k].out_mask[:] = 9
    ct = zg.Masks()
    C.memmove(C.byref(ct), C.byref(pm.ct), C.sizeof(ct))
    ct.fft_in[1] = ct.fft_out[1] = None
    ct.degred_in = ct.degred_out = None
    for k in (2, 3):
        ct.msm_in[k] = ct.msm_out[k] = None
    zk.api.deal_masks(pp, 1, log_m, g1row, None, 2000, ct)         # no G2 slot: no G2 generator needed
    pp.sync()
    for buf in (pm.fft[1].in_mask, pm.fft[1].out_mask, pm.degred.in_mask, pm.degred.out_mask):
        assert np.array_equal(buf.to_numpy(), fill)
    for k in (2, 3):
        assert (pm.msm[k].in_mask == 7).all() and (pm.msm[k].out_mask == 9).all()
    want = zk.FftMask.sample(pp, True, zg._root_of_unity("bn254", log_m + 1), 1, log_m, 2000)
    assert np.array_equal(pm.fft[0].in_mask.to_numpy(), want.in_mask.to_numpy())
    G = g1(BN254)
    single = zk.MsmMask.sample(pp, ZK_G1, g1row, 2000 + 7 + 4)
    assert all(G.eq(dec_jacobian(pp, pm.msm[4].out_mask[i]), dec_jacobian(pp, single.out_mask[i])) for i in range(pp.n))
    # a G2 slot without a G2 generator; one pointer of a pair; a curve without G2
    with pytest.raises(zk.ZkError):
        zk.api.deal_masks(pp, 1, log_m, g1row, None, 2000, pm.ct)
    half = zg.Masks()
    C.memmove(C.byref(half), C.byref(ct), C.sizeof(ct))
    half.fft_out[0] = None
    with pytest.raises(zk.ZkError):
        zk.api.deal_masks(pp, 1, log_m, g1row, g2row, 2000, half)
    p377 = ctx("bls12_377", 2)
    m377 = zg.Masks()
    pts = np.zeros((2, p377.n, 6 * p377.fq.nl), dtype=np.uint64)
    m377.msm_in[2], m377.msm_out[2] = pts[0].ctypes.data, pts[1].ctypes.data
    with pytest.raises(zk.ZkError):
        zk.api.deal_masks(p377, 1, log_m, enc_affine(p377, [g1(CURVES["bls12_377"]).gen])[0], pts[0][0][:4 * p377.fq.nl], 1, m377)
    m377.msm_in[2] = m377.msm_out[2] = None                      # ... and without it the G1 masks are dealt
    pts1 = np.zeros((2, p377.n, 3 * p377.fq.nl), dtype=np.uint64)    # n G1 points, packed as the prover reads them
    m377.msm_in[0], m377.msm_out[0] = pts1[0].ctypes.data, pts1[1].ctypes.data
    zk.api.deal_masks(p377, 1, log_m, enc_affine(p377, [g1(CURVES["bls12_377"]).gen])[0], None, 1, m377)
    G7 = g1(CURVES["bls12_377"])
    orc = _oracle_msm_mask("bls12_377", 2, False, 1 + 7)
    for i in range(p377.n):
        assert G7.eq(dec_jacobian(p377, pts1[0][i]), orc[i].in_mask), i
        assert G7.eq(dec_jacobian(p377, pts1[1][i]), orc[i].out_mask), i
    assert not pts.any()                                         # the rejected call wrote nothing


# ------------------------------------------------------------------------------------------------ the dealt masks work
def _proof_points(pp, o, shares):
    G1, G2 = g1(BN254), g2(BN254)
    pa, pb, pc = shares
    A = o.unpack2([dec_jacobian(pp, pa[i]) for i in range(o.n)], GroupOps(G1))[0]
    B = o.unpack2([dec_jacobian(pp, pb[i], True) for i in range(o.n)], GroupOps(G2))[0]
    Cc = o.unpack2([dec_jacobian(pp, pc[i]) for i in range(o.n)], GroupOps(G1))[0]
    return G1.to_affine(A), G2.to_affine(B), G1.to_affine(Cc)


def test_proofs_with_dealt_masks_equal_the_unmasked_proofs():
    r1, w = small_r1cs()
    pp, o = ctx("bn254", 2), opp("bn254", 2)
    P = BN254.r
    setup = zg.SetupScalars("bn254", r1, *[rand_fp(44, i, P) for i in range(5)])
    crs = zg.Crs(pp, setup)
    wit = zg.Witness(pp, "bn254", r1, w, seed=6)
    dealt = zg.ProofMasks.batch(pp, setup.log_m, 3000, 3)
    rs_ = [rand_fp(45, 2 * b, P) for b in range(3)]
    ss_ = [rand_fp(45, 2 * b + 1, P) for b in range(3)]
    plain = [_proof_points(pp, o, zg.prove(pp, crs, wit, rs_[b], ss_[b], seed=11 + 16 * b)) for b in range(3)]
    for b in range(3):
        assert _proof_points(pp, o, zg.prove(pp, crs, wit, rs_[b], ss_[b], masks=dealt[b], seed=11 + 16 * b)) == plain[b], b
    batch = zg.prove_batch(pp, crs, [wit] * 3, rs_, ss_, masks=dealt, seed=11)
    assert [_proof_points(pp, o, x) for x in batch] == plain
    # and the proof is the closed form of the oracle's prover
    okey = og.setup_scalars(BN254, r1, og.Trapdoor(*[rand_fp(44, i, P) for i in range(5)]))
    sa, sb, sc_ = og.prove_scalars(BN254, r1, okey, w, rs_[0], ss_[0])
    G1, G2 = g1(BN254), g2(BN254)
    assert plain[0] == (G1.to_affine(G1.mul(G1.from_affine(BN254.g1), sa)), G2.to_affine(G2.mul(G2.from_affine(BN254.g2), sb)),
                        G1.to_affine(G1.mul(G1.from_affine(BN254.g1), sc_)))


# ------------------------------------------------------------------------------------------------ production randomness
def test_deal_masks_outside_replay_mode_draws_fresh_masks_that_cancel():
    pp = zk.PackedSharingParams("bn254", 2)
    pp.set_option("rng_replay", 0)
    o = opp("bn254", 2)
    log_m = 4
    a, b = zg.ProofMasks.batch(pp, log_m, 5, 2), zg.ProofMasks.batch(pp, log_m, 5, 2)
    pp.sync()
    sets = a + b
    for i in range(4):
        for j in range(i + 1, 4):                                # same seed, different proofs and different calls
            for k in range(6):
                assert not np.array_equal(sets[i].fft[k].in_mask.to_numpy(), sets[j].fft[k].in_mask.to_numpy())
            for k in range(5):
                assert not np.array_equal(sets[i].msm[k].in_mask, sets[j].msm[k].in_mask)
                assert not np.array_equal(sets[i].msm[k].out_mask, sets[j].msm[k].out_mask)
    for k in range(5):                                           # no two masks of one set share their stream either
        for k2 in range(k + 1, 5):
            if (k == 2) == (k2 == 2):
                assert not np.array_equal(a[0].msm[k].in_mask, a[0].msm[k2].in_mask)
    # a masked d_msm with a dealt mask returns the unmasked result (dmsm_test.rs:50-51)
    m, l = 8, 2
    for group, G, is2, k in ((ZK_G1, g1(BN254), False, 0), (ZK_G2, g2(BN254), True, 2)):
        ops = GroupOps(G)
        y_pub = rand_vec(92, m, BN254.r)
        x_pub = [G.mul(G.from_affine(G.gen), j + 3) for j in range(m)]
        x_sh = od.transpose([o.det_pack(x_pub[j:j + l], ops) for j in range(0, m, l)])
        y_sh = od.transpose(od.pack_vec(y_pub, o, 93))
        bases = zk.DeviceBuffer.from_numpy(pp, np.concatenate([enc_affine(pp, G.batch_to_affine(v), is2) for v in x_sh]))
        scal = pp.upload_fr([v for vec in y_sh for v in vec])
        out = zk.d_msm(pp, group, bases, scal, m // l, b[1].msm[k])
        got = [dec_jacobian(pp, out[i], is2) for i in range(pp.n)]
        assert G.eq(o.unpack2(got, ops)[0], G.msm(G.batch_to_affine(x_pub), y_pub))
    pp.close()


# ------------------------------------------------------------------------------------------------ zk_groth16_deal_witness
@pytest.mark.parametrize("l", [2, 4])
def test_deal_witness_equals_the_direct_calls_on_padded_inputs(l):
    import random
    pp = ctx("bn254", l)
    p = BN254.r
    rng = random.Random(3)
    nv, ni, nc = 12, 3, 13                                       # nv - 1 = 11 and nv - ni = 9: no multiples of 2 or 4

    def lc():
        return [(rng.randrange(p), rng.randrange(nv)) for _ in range(rng.randrange(0, 5))]
    r = sc.R1CS(ni, nv - ni, [lc() for _ in range(nc)], [lc() for _ in range(nc)], [[] for _ in range(nc)])
    w = [1] + rand_vec(9, nv - 1, p)
    dev = circom.DeviceR1cs(pp, r)
    assert dev.log_m == 4
    m = 16
    w_d = pp.upload_fr(w)
    wit = zg.Witness(pp, "bn254", r, w_d, seed=40, dev_r1cs=dev)
    pp.sync()
    assert (wit.len_a, wit.len_w) == (-(-(nv - 1) // l), -(-(nv - ni) // l))
    # no host copy of the witness is made or kept
    assert not any(isinstance(v, (list, tuple)) and len(v) >= nv - ni for v in vars(wit).values())
    for k, d in enumerate(dev.qap(w_d)):
        pp._check(pp.lib.zk_bitrev(pp.h, d.ptr, dev.log_m, None))
        want = pp.pack(d, m // l, 40 + k, order=1)
        assert np.array_equal(wit.qap[k].to_numpy(), want.to_numpy()), k
    for vals, sd, got, ln in ((w[1:], 43, wit.a_share, wit.len_a), (w[ni:], 44, wit.ax_share, wit.len_w)):
        vals = list(vals) + [0] * (-len(vals) % l)
        want = pp.pack(pp.upload_fr(vals), len(vals) // l, sd)
        assert np.array_equal(got.to_numpy()[:pp.n * ln * pp.fr.nl], want.to_numpy()[:pp.n * ln * pp.fr.nl]), sd
    # the same shares from a host witness; the size query alone
    wit2 = zg.Witness(pp, "bn254", r, w, seed=40, dev_r1cs=dev)
    for x, y in zip(wit.qap + [wit.a_share, wit.ax_share], wit2.qap + [wit2.a_share, wit2.ax_share]):
        assert np.array_equal(x.to_numpy(), y.to_numpy())


def test_witness_from_a_device_buffer_never_downloads_it(monkeypatch):
    pp = ctx("bn254", 2)
    r1, w = small_r1cs()
    w_d = pp.upload_fr(w)
    calls = []
    real = zk.api.DeviceBuffer.to_numpy
    monkeypatch.setattr(zk.api.DeviceBuffer, "to_numpy", lambda self, *a, **k: calls.append(self) or real(self, *a, **k))
    wit = zg.Witness(pp, "bn254", r1, w_d, seed=6)
    assert calls == []
    monkeypatch.undo()
    want = zg.Witness(pp, "bn254", r1, w, seed=6)
    assert np.array_equal(wit.a_share.to_numpy(), want.a_share.to_numpy())


# ------------------------------------------------------------------------------------------------ two streams
def test_deal_masks_on_two_streams_at_once_equals_the_serial_results():
    import torch
    pp = zk.PackedSharingParams("bn254", 2)
    log_m, nb = 10, 3

    def snap(sets):
        out = []
        for pm in sets:
            out += [x.to_numpy().copy() for f in pm.fft for x in (f.in_mask, f.out_mask)]
            out += [pm.degred.in_mask.to_numpy().copy(), pm.degred.out_mask.to_numpy().copy()]
            out += [x.copy() for mm in pm.msm for x in (mm.in_mask, mm.out_mask)]
        return out

    serial = []
    for i in range(2):
        serial.append(snap(zg.ProofMasks.batch(pp, log_m, 7000 + 100 * i, nb)))
        pp.sync()
    streams = [torch.cuda.Stream() for _ in range(2)]
    for rep in range(3):
        sets = [zg.ProofMasks.batch(pp, log_m, 7000 + 100 * i, nb, stream=streams[i].cuda_stream) for i in range(2)]
        for st in streams:
            st.synchronize()
        for i in range(2):
            for got, want in zip(snap(sets[i]), serial[i]):
                assert np.array_equal(got, want), (rep, i)
    pp.close()
