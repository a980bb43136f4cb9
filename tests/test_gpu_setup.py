"""zk_groth16_setup_scalars (`pytest -m gpu`): the circuit-specific setup on the device against oracle.groth16.setup_scalars
through DeviceSetup.to_host().  Everything is an integer: every comparison is exact equality."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import groth16 as zg
from zksaas_amd import sha256_circuit as sc
from zksaas_amd._lib import ZkError
from zksaas_amd.api import DeviceBuffer
from zksaas_amd.circom import DeviceR1cs
from oracle import groth16 as og
from oracle.curve import g1, g2
from oracle.field import Domain
from oracle.params import BN254, CURVES
from oracle.prng import rand_fp

from gpu_util import ctx
from test_oracle_groth16 import small_r1cs

BOTH = ["bn254", "bls12_381"]
VECS = ("a_query", "b_query", "l_query", "h_query", "gamma_abc")
ZK_ERR_GENERIC, ZK_ERR_BAD_INPUT = 1, 4
MARK = 0xA5A5A5A5A5A5A5A5


def trapdoor(seed, p):
    return [rand_fp(seed, i, p) for i in range(5)]


def device_r1cs(pp, r1):
    return DeviceR1cs(pp, r1).upload_c(r1)


def assert_equals_oracle(curve, r1, td, got=None):
    pp = ctx(curve)
    want = og.setup_scalars(CURVES[curve], r1, og.Trapdoor(*td))
    got = got or zg.DeviceSetup(pp, device_r1cs(pp, r1), *td).to_host()
    for k in VECS:
        assert getattr(got, k) == getattr(want, k), k
    return want


def random_r1cs(seed, nc, ni, nw, p):
    """every row of A, B and C holds one to three random terms over the nv wires"""
    nv = ni + nw
    mats = []
    for k in range(3):
        rows = []
        for i in range(nc):
            cnt = 1 + rand_fp(seed + k, 3 * i, 3)
            rows.append([(rand_fp(seed + k, 3 * i + 1 + t, p), rand_fp(seed + 10 + k, 3 * i + t, nv)) for t in range(cnt)])
        mats.append(rows)
    return og.R1CS(ni, nw, *mats)


# ------------------------------------------------------------------------------------------------ 1. small circuit
@pytest.mark.parametrize("curve", BOTH)
def test_small_r1cs_equals_the_oracle(curve):
    r1, _ = small_r1cs()               # (the matrices hold small coefficients: the same R1CS over either field)
    assert_equals_oracle(curve, r1, trapdoor(42, CURVES[curve].r))


# ------------------------------------------------------------------------------------------------ 2. domain edges
@pytest.mark.parametrize("nc,ni,nw", [(1, 1, 2), (14, 2, 5), (15, 2, 5), (5, 1, 6), (5, 4, 0)],
                         ids=["m2", "power_of_two", "one_past_a_power", "ni1", "ni_eq_nv"])
def test_domain_edges(nc, ni, nw):
    p = BN254.r
    r1 = random_r1cs(100 + nc, nc, ni, nw, p)
    want = assert_equals_oracle("bn254", r1, trapdoor(50 + nc, p))
    assert want.domain.size == {2: 2, 16: 16, 17: 32, 6: 8, 9: 16}[nc + ni]
    assert len(want.l_query) == nw


# ------------------------------------------------------------------------------------------------ 3. matrix shapes
def test_matrix_shapes():
    """an empty row, a wire no row mentions (in each of A, B, C; wire 1 is an instance wire: its a_query is u_{nc+1} alone),
    the same wire twice in one row, coefficients 0, 1 and p - 1, an all-empty C"""
    p = BN254.r
    A = [[(1, 0), (p - 1, 2)], [], [(5, 3), (7, 3)], [(0, 4), (1, 5)], [(2, 0)], [(3, 2), (p - 1, 2)]]
    B = [[(1, 1)], [(p - 1, 1), (1, 1)], [], [(0, 0)], [(1, 6), (1, 6), (1, 6)], [(4, 2)]]
    Cm = [[] for _ in range(6)]
    r1 = og.R1CS(2, 6, A, B, Cm)
    td = trapdoor(61, p)
    want = assert_equals_oracle("bn254", r1, td)
    u = og.lagrange_coeffs_at(want.domain, td[4])
    assert want.a_query[1] == u[6 + 1] and want.a_query[6] == 0 and want.a_query[7] == 0
    assert want.b_query[7] == 0 and want.b_query[3] == 0
    assert want.a_query[3] == 12 * u[2] % p                       # both terms of the doubled wire count
    assert want.b_query[1] == (u[0] + 0 * u[1]) % p               # 1 and p - 1 cancel in row 1


# ------------------------------------------------------------------------------------------------ 4. / 5. heavy columns
HEAVY_NC = 3000


@functools.lru_cache(maxsize=None)
def heavy_case():
    """nc = 3000, m = 4096: wire 0 in every row of A, B and C, wire 1 in every second row, wire 2 in exactly SETUP_HEAVY_MIN
    rows of A and wire 3 in one more; every other wire in two rows"""
    p = BN254.r
    T = zg.SETUP_HEAVY_MIN
    nc, ni = HEAVY_NC, 2
    mats = []
    for k in range(3):
        rows = []
        for i in range(nc):
            row = [(rand_fp(70 + k, 4 * i, p), 0), (rand_fp(70 + k, 4 * i + 1, p), 4 + i // 2)]
            if i % 2 == 0:
                row.append((rand_fp(70 + k, 4 * i + 2, p), 1))
            if k == 0 and i < T:
                row.append((rand_fp(70 + k, 4 * i + 3, p), 2))
            if k == 0 and 100 <= i < 100 + T + 1:
                row.append((rand_fp(70 + k, 4 * i + 3, p), 3))
            rows.append(row)
        mats.append(rows)
    r1 = og.R1CS(ni, 2 + nc // 2, *mats)
    td = trapdoor(71, p)
    return r1, td, og.setup_scalars(BN254, r1, og.Trapdoor(*td))


def test_heavy_columns_equal_the_oracle():
    assert HEAVY_NC > zg.SETUP_HEAVY_MIN           # wire 0 (3000 rows) and wire 1 (1500) take the workgroup path
    assert HEAVY_NC // 2 > 4 * zg.SETUP_HEAVY_MIN
    r1, td, want = heavy_case()
    assert want.domain.size == 4096
    cols = [sum(1 for row in r1.a for _, j in row if j == wire) for wire in range(4)]
    assert cols == [HEAVY_NC, HEAVY_NC // 2, zg.SETUP_HEAVY_MIN, zg.SETUP_HEAVY_MIN + 1]
    pp = ctx("bn254")
    got = zg.DeviceSetup(pp, device_r1cs(pp, r1), *td).to_host()
    for k in VECS:
        assert getattr(got, k) == getattr(want, k), k


def raw_vectors(ds):
    return [getattr(ds, k).to_numpy().tobytes() for k in VECS]


def test_heavy_columns_are_deterministic_across_calls_and_streams():
    import torch
    r1, td, _ = heavy_case()
    pp = ctx("bn254")
    dev = device_r1cs(pp, r1)
    st = torch.cuda.Stream()
    first = raw_vectors(zg.DeviceSetup(pp, dev, *td))
    second = raw_vectors(zg.DeviceSetup(pp, dev, *td))
    other = zg.DeviceSetup(pp, dev, *td, stream=st.cuda_stream)
    pp.sync(st.cuda_stream)
    assert first == second
    assert first == raw_vectors(other)


# ------------------------------------------------------------------------------------------------ 6. tails and NULLs
def raw_call(pp, dev, r1, td, tail, bufs, log_m=None):
    mats = [b.ptr for mat in (dev._mats[0], dev._mats[1], dev.c_mat) for b in mat]
    t = np.ascontiguousarray(pp.fr.encode(list(td)))
    pp._check(pp.lib.zk_groth16_setup_scalars(pp.h, *mats, r1.num_variables, r1.num_constraints, r1.num_instance_variables,
                                              dev.log_m if log_m is None else log_m, t.ctypes.data, tail,
                                              *[None if b is None else b.ptr for b in bufs], None))


def test_tails_are_zero_guards_untouched_and_null_outputs_skipped():
    p = BN254.r
    r1, _ = small_r1cs()
    pp = ctx("bn254")
    dev = device_r1cs(pp, r1)
    td = trapdoor(81, p)
    nv, ni, m, nl = r1.num_variables, r1.num_instance_variables, 1 << dev.log_m, pp.fr.nl
    tail, guard = 3, 2
    lens = [nv, nv, nv - ni, m, ni]
    tails = [tail, tail, tail, tail, 0]                 # (order of the ABI: a, b, l, h, gamma_abc; gamma_abc has no tail)

    def marked():
        return [DeviceBuffer.from_numpy(pp, np.full((n_ + t_ + guard) * nl, MARK, dtype=np.uint64)) for n_, t_ in zip(lens, tails)]

    full = marked()
    raw_call(pp, dev, r1, td, tail, full)
    want = og.setup_scalars(BN254, r1, og.Trapdoor(*td))
    vals = [want.a_query, want.b_query, want.l_query, want.h_query, want.gamma_abc]
    got = [b.to_numpy() for b in full]
    for arr, n_, t_, v in zip(got, lens, tails, vals):
        assert pp.fr.decode(arr[:n_ * nl]) == v
        assert not arr[n_ * nl:(n_ + t_) * nl].any()
        assert (arr[(n_ + t_) * nl:] == MARK).all()
    part = marked()
    raw_call(pp, dev, r1, td, tail, [None] + part[1:])
    for k in range(1, 5):
        assert (part[k].to_numpy() == got[k]).all(), VECS[k]
    only_h = marked()
    raw_call(pp, dev, r1, td, tail, [None, None, None, only_h[3], None])
    assert (only_h[3].to_numpy() == got[3]).all()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_context_usable():
    p = BN254.r
    r1, _ = small_r1cs()
    pp = ctx("bn254")
    dev = device_r1cs(pp, r1)
    td = trapdoor(91, p)
    nv, ni, m = r1.num_variables, r1.num_instance_variables, 1 << dev.log_m

    def valid_call_succeeds():
        assert_equals_oracle("bn254", r1, td, zg.DeviceSetup(pp, dev, *td).to_host())

    def refused(code, word, call):
        with pytest.raises(ZkError) as ei:
            call()
        assert ei.value.code == code, ei.value
        assert word in ei.value.msg, ei.value.msg
        valid_call_succeeds()

    # a wire index == nv in B
    bad_rows = [list(row) for row in r1.b]
    bad_rows[3] = bad_rows[3] + [(1, nv)]
    bad_dev = DeviceR1cs(pp, og.R1CS(ni, nv - ni, r1.a, bad_rows, r1.c)).upload_c(r1)
    refused(ZK_ERR_GENERIC, "wire index", lambda: zg.DeviceSetup(pp, bad_dev, *td))
    # 2^log_m < nc + ni
    outs = [pp.alloc_fr(nv + 2), pp.alloc_fr(nv + 2), pp.alloc_fr(nv + 2), pp.alloc_fr(m + 2), pp.alloc_fr(ni)]
    refused(ZK_ERR_BAD_INPUT, "domain", lambda: raw_call(pp, dev, r1, td, 0, outs, log_m=dev.log_m - 1))
    # degenerate trapdoors: alpha, beta, gamma, delta, tau
    w = Domain(BN254, m).group_gen
    w2 = Domain(BN254, 2 * m).group_gen
    assert pow(w2, m, p) == p - 1 and w2 * w2 % p == w          # the odd 2m-th root: x_0 - 1 = 0 in h_0's denominator
    a, b, g, d, t = td
    refused(ZK_ERR_BAD_INPUT, "gamma", lambda: zg.DeviceSetup(pp, dev, a, b, 0, d, t))
    refused(ZK_ERR_BAD_INPUT, "delta", lambda: zg.DeviceSetup(pp, dev, a, b, g, 0, t))
    for bad_tau in (0, 1, w, w2):
        refused(ZK_ERR_BAD_INPUT, "tau", lambda: zg.DeviceSetup(pp, dev, a, b, g, d, bad_tau))


# ------------------------------------------------------------------------------------------------ 8. end to end
def _decode_proof(pp, aff):
    v = pp.fq.decode(np.asarray(aff).reshape(-1, pp.fq.nl))
    return (v[0], v[1]), ((v[2], v[3]), (v[4], v[5])), (v[6], v[7])


def test_small_circuit_from_device_setup_to_a_verified_proof():
    p = BN254.r
    r1, w = small_r1cs()
    pp = ctx("bn254")
    td = trapdoor(95, p)
    dsetup = zg.DeviceSetup(pp, device_r1cs(pp, r1), *td)
    crs = zg.Crs.from_device_setup(pp, dsetup)
    wit = zg.Witness(pp, "bn254", r1, w, seed=5)
    r, s = rand_fp(96, 0, p), rand_fp(96, 1, p)
    aff, _ = zg.reconstruct(pp, zg.prove(pp, crs, wit, r, s, seed=9), want_bytes=False)
    # the closed form a trapdoor holder evaluates
    okey = og.setup_scalars(BN254, r1, og.Trapdoor(*td))
    sa, sb, sc_ = og.prove_scalars(BN254, r1, okey, w, r, s)
    G1, G2 = g1(BN254), g2(BN254)
    A, B, Cc = _decode_proof(pp, aff)
    assert G1.eq(G1.from_affine(A), G1.mul(G1.from_affine(BN254.g1), sa))
    assert G2.eq(G2.from_affine(B), G2.mul(G2.from_affine(BN254.g2), sb))
    assert G1.eq(G1.from_affine(Cc), G1.mul(G1.from_affine(BN254.g1), sc_))
    # the pairing check, with the verifying key read from the device setup
    pvk = zg.PreparedVk(pp, zg.verifying_key(pp, dsetup))
    assert zg.verify(pp, pvk, [aff], [[w[1]]]) == [True]
    assert zg.verify(pp, pvk, [aff], [[(w[1] + 1) % p]]) == [False]
    # the packed CRS shares are those of the host setup, byte for byte
    host = zg.Crs(pp, zg.SetupScalars("bn254", r1, *td))
    for k in ("s", "h", "v", "w", "u"):
        assert getattr(crs, k).to_numpy().tobytes() == getattr(host, k).to_numpy().tobytes(), k
    assert (crs.len_a, crs.len_w, crs.len_u) == (host.len_a, host.len_w, host.len_u)
    assert crs.s1.tobytes() == host.s1.tobytes() and crs.s2.tobytes() == host.s2.tobytes()
    assert zg.verifying_key(pp, dsetup) == zg.verifying_key(pp, zg.SetupScalars("bn254", r1, *td))


# ------------------------------------------------------------------------------------------------ 9. SHA-256 fixture
def test_sha256_fixture_setup_equals_the_host_setup_and_its_proof_verifies():
    p = BN254.r
    r1, w = sc.build(1, 2, p)
    pp = ctx("bn254")
    td = trapdoor(42, p)
    host = zg.SetupScalars("bn254", r1, *td)
    dsetup = zg.DeviceSetup(pp, device_r1cs(pp, r1), *td)
    assert dsetup.log_m == 15
    got = dsetup.to_host()
    for k in VECS:
        assert getattr(got, k) == getattr(host, k), k
    crs = zg.Crs.from_device_setup(pp, dsetup)
    wit = zg.Witness(pp, "bn254", r1, w, seed=7)
    aff, _ = zg.reconstruct(pp, zg.prove(pp, crs, wit, rand_fp(43, 0, p), rand_fp(43, 1, p), seed=11), want_bytes=False)
    pvk = zg.PreparedVk(pp, zg.verifying_key(pp, dsetup))
    assert zg.verify(pp, pvk, [aff], [[w[1]]]) == [True]
