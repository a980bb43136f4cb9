// Kernels and host side of the verifier (pairing.hpp), generic over the curve; instantiated in pairing_<curve>.hip.
//
// Miller loop (ark-ec `Bn::multi_miller_loop` / `Bls12::multi_miller_loop`, without their precomputed line tables): one
// (P, Q) pair per group of PAIRING_GW lanes.  The running G2 point stays in homogeneous projective coordinates and the
// doubling / addition steps are the inversion-free formulas of Costello, Lange and Naehrig ("Faster pairing computations
// on curves with high-degree twists", the ones ark-ec's `doubling_step` / `addition_step` use); every lane of the group
// runs them on its own copy (they are a dozen Fq2 products against the 9 per lane -- 6 of the squaring, 3 of the line --
// of the Fq12 work of the same step, and no exchange is needed), the Fq12 accumulator is lane-split (tower.hpp).  A line
// is scaled by elements of Fq2, which the final exponentiation kills.
//
// Final exponentiation: easy part (q^6 - 1)(q^2 + 1) with the one inversion, then the hard exponent as four base-q
// digits d_0..d_3 (pairing_params.hpp) by a joint square-and-multiply over g_i = f^(q^i): one cyclotomic squaring per bit
// and at most two products with entries of the tables {g_0, g_1, g_0 g_1} and {g_2, g_3, g_2 g_3}.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "ec.hpp"
#include "pairing.hpp"
#include "tower.hpp"

namespace zk {

template <class PP>
struct PairingDev {
  using T = Tower<PP>;
  using L12 = Lane12<PP>;
  using Fq = typename T::Fq;
  using F2 = typename T::F2;
  static constexpr int N = Fq::N;
  struct G2Proj {
    F2 x, y, z;
  };
  struct HardDigits {
    uint32_t d[4][N];
  };

  // x / 2: (x + p) / 2 when x is odd (also the Montgomery form of half the value)
  static ZK_D Fq half(const Fq& a) {
    const uint32_t mask = 0u - (a.v[0] & 1u);
    uint32_t t[N];
    unsigned c = 0;
#pragma unroll
    for (int i = 0; i < N; i++) t[i] = __builtin_addc(a.v[i], PP::FqP::MOD[i] & mask, c, &c);
    Fq r;
#pragma unroll
    for (int i = 0; i < N - 1; i++) r.v[i] = (t[i] >> 1) | (t[i + 1] << 31);
    r.v[N - 1] = (t[N - 1] >> 1) | ((uint32_t)c << 31);
    return r;
  }
  static ZK_D F2 half2(const F2& a) { return {half(a.c0), half(a.c1)}; }

  // R <- 2R; the tangent at R evaluated at P as l0 + ls w^S + l3 w^3
  static __device__ __attribute__((noinline)) void dbl_step(G2Proj& R, const Fq& xp, const Fq& yp, F2& l0, F2& ls, F2& l3) {
    const F2 a = half2(R.x * R.y), b = R.y.sqr(), c = R.z.sqr();
    const F2 e = T::f2_const(PP::TWIST_B) * (c.dbl() + c), f = e.dbl() + e;
    const F2 g = half2(b + f), h = (R.y + R.z).sqr() - (b + c);
    const F2 i = e - b, j = R.x.sqr(), e2 = e.sqr();
    R.x = a * (b - f);
    R.y = g.sqr() - (e2.dbl() + e2);
    R.z = b * h;
    const F2 j3 = T::scale2(j.dbl() + j, xp), nh = T::scale2(h.neg(), yp);
    ls = j3;
    if constexpr (PP::TWIST_D) l0 = nh, l3 = i;
    else l0 = i, l3 = nh;
  }
  // R <- R + Q (Q affine, not the identity); the chord evaluated at P
  static __device__ __attribute__((noinline)) void add_step(G2Proj& R, const F2& qx, const F2& qy, const Fq& xp, const Fq& yp,
                                                            F2& l0, F2& ls, F2& l3) {
    const F2 th = R.y - qy * R.z, la = R.x - qx * R.z;
    const F2 c = th.sqr(), d = la.sqr(), e = la * d, f = R.z * c, g = R.x * d;
    const F2 h = e + f - g.dbl();
    const F2 j = th * qx - la * qy;
    R.y = th * (g - h) - e * R.y;
    R.x = la * h;
    R.z = R.z * e;
    const F2 lay = T::scale2(la, yp);
    ls = T::scale2(th.neg(), xp);
    if constexpr (PP::TWIST_D) l0 = lay, l3 = j;
    else l0 = j, l3 = lay;
  }

  // f_{LOOP, Q}(P) (with the two Frobenius lines of a BN curve; conjugated for a negative parameter); 1 for an identity
  static ZK_D F2 miller(const L12& L, const Affine<Fq>& P, const Affine<F2>& Q) {
    F2 f = L.one(), l0, ls, l3;
    G2Proj R{Q.x, Q.y, F2::one()};
#pragma unroll 1
    for (int b = PP::LOOP_BITS - 2; b >= 0; b--) {
      dbl_step(R, P.x, P.y, l0, ls, l3);
      f = L.mul_by_line(L.sqr(f), l0, ls, l3);
      if (((b < 64 ? PP::LOOP[0] : PP::LOOP[1]) >> (b & 63)) & 1) {
        add_step(R, Q.x, Q.y, P.x, P.y, l0, ls, l3);
        f = L.mul_by_line(f, l0, ls, l3);
      }
    }
    if constexpr (PP::BN_FROB_LINES) {
      // Q1 = pi(Q), -Q2 = -pi^2(Q) on the twist
      const F2 q1x = T::conj2(Q.x) * T::template frob_coeff<1, 2>(), q1y = T::conj2(Q.y) * T::template frob_coeff<1, 3>();
      add_step(R, q1x, q1y, P.x, P.y, l0, ls, l3);
      f = L.mul_by_line(f, l0, ls, l3);
      const F2 q2x = Q.x * T::template frob_coeff<2, 2>(), q2y = (Q.y * T::template frob_coeff<2, 3>()).neg();
      add_step(R, q2x, q2y, P.x, P.y, l0, ls, l3);
      f = L.mul_by_line(f, l0, ls, l3);
    }
    if constexpr (PP::LOOP_NEG) f = L.conj(f);
    return L12::sel(P.is_identity() || Q.is_identity(), L.one(), f);
  }

  static ZK_D F2 final_exp(const L12& L, const F2& f, const HardDigits& hd) {
    const F2 f1 = L.mul(L.conj(f), L.inverse(f));                 // ^(q^6 - 1)
    const F2 g0 = L.mul(L.template frobenius<2>(f1), f1);         // ^(q^2 + 1): in the cyclotomic subgroup from here on
    const F2 g1 = L.template frobenius<1>(g0), g2 = L.template frobenius<2>(g0), g3 = L.template frobenius<3>(g0);
    const F2 g01 = L.mul(g0, g1), g23 = L.mul(g2, g3);
    F2 acc = L.one();
#pragma unroll 1
    for (int b = PP::HARD_BITS - 1; b >= 0; b--) {
      acc = L.cyclotomic_sqr(acc);
      const int w = b >> 5, s = b & 31;
      const uint32_t i0 = ((hd.d[0][w] >> s) & 1u) | (((hd.d[1][w] >> s) & 1u) << 1);
      const uint32_t i1 = ((hd.d[2][w] >> s) & 1u) | (((hd.d[3][w] >> s) & 1u) << 1);
      if (i0) acc = L.mul(acc, i0 == 1 ? g0 : i0 == 2 ? g1 : g01);      // (uniform: the digits are kernel arguments)
      if (i1) acc = L.mul(acc, i1 == 1 ? g2 : i1 == 2 ? g3 : g23);
    }
    return acc;
  }
};

// one (P, Q) pair per lane group -> its Miller value, [npairs][6] Fq2 in memory order
template <class PP>
__global__ __launch_bounds__(256) void pairing_miller_kernel(const Affine<typename Tower<PP>::Fq>* __restrict__ P,
                                                             const Affine<typename Tower<PP>::F2>* __restrict__ Q,
                                                             size_t npairs, typename Tower<PP>::F2* __restrict__ out) {
  using D = PairingDev<PP>;
  const typename D::L12 L = D::L12::here();
  size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / PAIRING_GW;
  const bool live = g < npairs;
  if (!live) g = npairs - 1;                    // whole groups repeat the last pair and do not store
  const typename D::F2 f = D::miller(L, P[g], Q[g]);
  if (live) L.store(out + g * 6, f);
}

// out[i] = final_exp(prod_{t < k} mill[i][t]); with `expect`: ok[i] = valid[i] && out[i] == expect
template <class PP>
__global__ __launch_bounds__(256) void pairing_final_exp_kernel(const typename Tower<PP>::F2* __restrict__ mill, size_t k,
                                                                size_t count, typename PairingDev<PP>::HardDigits hd,
                                                                typename Tower<PP>::F2* __restrict__ gt_out,
                                                                const typename Tower<PP>::F2* __restrict__ expect,
                                                                const uint8_t* __restrict__ valid, uint8_t* __restrict__ ok) {
  using D = PairingDev<PP>;
  using F2 = typename D::F2;
  const typename D::L12 L = D::L12::here();
  size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / PAIRING_GW;
  const bool live = g < count;
  if (!live) g = count - 1;
  F2 f = L.load(mill + g * k * 6);
#pragma unroll 1
  for (size_t t = 1; t < k; t++) f = L.mul(f, L.load(mill + (g * k + t) * 6));
  const F2 r = D::final_exp(L, f, hd);
  if (live && gt_out) L.store(gt_out + g * 6, r);
  if (expect) {
    const bool same = r == L.load(expect);      // (lanes 6, 7 hold copies of coefficients 0, 1)
    const unsigned long long m = __ballot(same);
    if (live && (threadIdx.x & (PAIRING_GW - 1)) == 0) ok[g] = (uint8_t)(valid[g] && ((m >> L.base) & 0xffull) == 0xffull);
  }
}

// parity access to the lane-split tower (zk_fq12_selftest)
template <class PP>
__global__ __launch_bounds__(256) void pairing_fq12_selftest_kernel(int op, const typename Tower<PP>::F2* __restrict__ a,
                                                                    const typename Tower<PP>::F2* __restrict__ b, size_t len,
                                                                    typename Tower<PP>::F2* __restrict__ out) {
  using D = PairingDev<PP>;
  using F2 = typename D::F2;
  const typename D::L12 L = D::L12::here();
  size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / PAIRING_GW;
  const bool live = g < len;
  if (!live) g = len - 1;
  const F2 x = L.load(a + g * 6);
  F2 r;
  switch (op) {                                   // uniform
    case 0: r = L.mul(x, L.load(b + g * 6)); break;
    case 1: r = L.sqr(x); break;
    case 2: r = L.inverse(x); break;
    case 3: r = L.conj(x); break;
    case 4: r = L.template frobenius<1>(x); break;
    case 5: r = L.template frobenius<2>(x); break;
    case 6: r = L.template frobenius<3>(x); break;
    case 7: r = L.cyclotomic_sqr(x); break;
    default: r = L.mul_by_line(x, b[g * 6], b[g * 6 + 1], b[g * 6 + 2]); break;
  }
  if (live) L.store(out + g * 6, r);
}

// A | B | C of one proof as zk_groth16_reconstruct writes it
template <class Fq, class F2>
struct ProofAffine {
  Affine<Fq> A;
  Affine<F2> B;
  Affine<Fq> C;
};

// zk_groth16_vk_prepare: table[t][k] = 2^k abc[t + 1], k < the bits of Fr, one lane per input (once per key).  With it the
// input combination of a proof is a sum of table entries, spread over the lanes of a wave, instead of a double-and-add chain.
template <class Fq, int BITS>
__global__ __launch_bounds__(64) void pairing_abc_table_kernel(const Affine<Fq>* __restrict__ abc, size_t n_inputs,
                                                               XYZZ<Fq>* __restrict__ table) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_inputs) return;
  XYZZ<Fq> p = XYZZ<Fq>::from_affine(abc[t + 1]);
#pragma unroll 1
  for (int k = 0; k < BITS; k++) {
    table[t * BITS + k] = p;
    p = xyzz_dbl_ni(p);
  }
}

template <class Fq>
__device__ XYZZ<Fq> xyzz_from_lane(const XYZZ<Fq>& p, int src) {
  XYZZ<Fq> r;
#pragma unroll
  for (int i = 0; i < Fq::N; i++) {
    r.X.v[i] = (uint32_t)__shfl((int)p.X.v[i], src);
    r.Y.v[i] = (uint32_t)__shfl((int)p.Y.v[i], src);
    r.ZZ.v[i] = (uint32_t)__shfl((int)p.ZZ.v[i], src);
    r.ZZZ.v[i] = (uint32_t)__shfl((int)p.ZZZ.v[i], src);
  }
  return r;
}

// ark-groth16 prepare_inputs + the three pairs of verify_proof, one proof per wave:
//   acc = abc[0] + sum_i x_i abc[i + 1];  pairs (A, B), (acc, -gamma), (C, -delta);  valid = every coordinate canonical and
//   A, C on G1's curve, B on the twist (the identity counts as on the curve; no subgroup check, as in verify_proof).
// Lane l sums the table entries 2^k abc[i + 1] of the set bits k = l, l + 64, ... of every x_i; six exchange rounds fold the
// 64 partial sums (the additions themselves may diverge, the exchanges are made with the wave converged); lane 0 finishes.
template <class PP, class FrP>
__global__ __launch_bounds__(64) void pairing_verify_prep_kernel(
    const ProofAffine<typename Tower<PP>::Fq, typename Tower<PP>::F2>* __restrict__ proofs, const Fp<FrP>* __restrict__ inputs,
    size_t n_inputs, const Affine<typename Tower<PP>::Fq>* __restrict__ abc,
    const XYZZ<typename Tower<PP>::Fq>* __restrict__ table, const Affine<typename Tower<PP>::F2>* __restrict__ neg_gamma,
    const Affine<typename Tower<PP>::F2>* __restrict__ neg_delta, int b1, size_t count, Affine<typename Tower<PP>::Fq>* __restrict__ P,
    Affine<typename Tower<PP>::F2>* __restrict__ Q, uint8_t* __restrict__ valid) {
  using T = Tower<PP>;
  using Fq = typename T::Fq;
  using Fr = Fp<FrP>;
  constexpr int BITS = FrP::BITS;
  const size_t i = blockIdx.x;                    // (the grid is `count` workgroups of one wave)
  const int lane = (int)threadIdx.x;
  XYZZ<Fq> acc = XYZZ<Fq>::identity();
#pragma unroll 1
  for (size_t t = 0; t < n_inputs; t++) {
    const Fr x = inputs[i * n_inputs + t].from_mont();
#pragma unroll 1
    for (int k = lane; k < BITS; k += 64)
      if ((x.v[k >> 5] >> (k & 31)) & 1u) acc = xyzz_add_ni(acc, table[t * BITS + k]);
  }
#pragma unroll 1
  for (int off = 32; off >= 1; off >>= 1) {
    const XYZZ<Fq> other = xyzz_from_lane(acc, (lane + off) & 63);
    acc = xyzz_add_ni(acc, other);                // (lanes >= off compute sums nobody reads)
  }
  if (lane != 0) return;
  acc = xyzz_add_ni(acc, XYZZ<Fq>::from_affine(abc[0]));
  const auto pr = proofs[i];
  P[3 * i] = pr.A;
  P[3 * i + 1] = xyzz_to_affine(acc);
  P[3 * i + 2] = pr.C;
  Q[3 * i] = pr.B;
  Q[3 * i + 1] = *neg_gamma;
  Q[3 * i + 2] = *neg_delta;
  const Fq bq = Fq::from_u64((uint64_t)b1);
  auto on_g1 = [&](const Affine<Fq>& p) {
    if (!p.x.is_canonical() || !p.y.is_canonical()) return false;
    return p.is_identity() || Fq::mul_ni(p.y, p.y) == Fq::mul_ni(Fq::mul_ni(p.x, p.x), p.x) + bq;
  };
  bool okb = pr.B.x.c0.is_canonical() && pr.B.x.c1.is_canonical() && pr.B.y.c0.is_canonical() && pr.B.y.c1.is_canonical();
  okb = okb && (pr.B.is_identity() || pr.B.y.sqr() == pr.B.x.sqr() * pr.B.x + T::f2_const(PP::TWIST_B));
  valid[i] = (uint8_t)(on_g1(pr.A) && on_g1(pr.C) && okb);
}

}  // namespace zk
#include "pairing_rlc.hpp"
#include "subgroup_impl.hpp"
namespace zk {

#define ZK_PAIR_HIP(expr)                                \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return e->hip_fail(_e, #expr); \
  } while (0)

template <class PP, class FrP, int CURVE, int B1>
class PairingImpl : public IPairing {
  using T = Tower<PP>;
  using D = PairingDev<PP>;
  using Fq = typename T::Fq;
  using F2 = typename T::F2;
  using Fr = Fp<FrP>;
  // Working memory per device, kept between calls and grown on demand (a hipFree synchronises the device: freeing seven
  // buffers at the end of every call would also make a call whose wait deadline passed block until the device drains).
  // A call holds the workspace of its device from its first launch to the end of its wait.  Never destroyed: the HIP
  // runtime may be gone when static destructors run.
  struct Workspace {
    std::mutex mu;
    DevBuf proofs, inputs, P, Q, mill, valid, ok;
    // zk_groth16_verify_all: points (r_i C_i, the levels of the two sums), Fr (r_i, s and s_t), bytes (validity and its
    // levels, the folded byte, the verdict), Fq12 (the group products, the value after the final exponentiation)
    DevBuf rlc_pts, rlc_fr, rlc_bytes, rlc_gt;
    // the bytes verifiers: the wire bytes (proofs, then inputs) and the staged verdicts (three per proof, then one per proof)
    DevBuf wire, stage_ok;
    uint8_t host_ok = 0;              // where the verdict and the value land: not the caller's memory, which a call whose
    F2 host_gt[6];                    // wait deadline passed has already given back
  };
  std::mutex ws_mu_;
  std::map<int, Workspace*> ws_;
  Workspace& workspace(int device) {
    std::lock_guard<std::mutex> g(ws_mu_);
    Workspace*& w = ws_[device];
    if (!w) w = new Workspace();
    return *w;
  }
  static constexpr int GROUPS_PER_BLOCK = 256 / PAIRING_GW;
  static unsigned blocks(size_t groups) { return (unsigned)((groups + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK); }
  static typename D::HardDigits digits() {
    typename D::HardDigits hd;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < Fq::N; j++) hd.d[i][j] = PP::HARD[i][j];
    return hd;
  }
  // the end of everything enqueued on st, within the context's wait deadline
  static int wait(IEngine* e, hipStream_t st, const char* what) {
    hipEvent_t ev;
    ZK_PAIR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t h = hipEventRecord(ev, st);
    if (h == hipSuccess) h = e->event_wait(ev);
    (void)hipEventDestroy(ev);
    if (h == hipErrorNotReady) return e->wedge(std::string(what) + ": the wait deadline passed (wait_deadline_ms)");
    return h == hipSuccess ? ZK_OK : e->hip_fail(h, what);
  }
  // Miller loops of npairs = count * k pairs, the product of every k and the final exponentiations
  int launch(IEngine* e, const void* p_d, const void* q_d, size_t k, size_t count, F2* mill, F2* gt_out, const F2* expect,
             const uint8_t* valid, uint8_t* ok, hipStream_t st) {
    {
      ProfScope ps(e->prof, PROF_MILLER, st, (double)(count * k));
      hipLaunchKernelGGL(pairing_miller_kernel<PP>, dim3(blocks(count * k)), dim3(256), 0, st, (const Affine<Fq>*)p_d,
                         (const Affine<F2>*)q_d, count * k, mill);
    }
    {
      ProfScope ps(e->prof, PROF_FINAL_EXP, st, (double)count);
      hipLaunchKernelGGL(pairing_final_exp_kernel<PP>, dim3(blocks(count)), dim3(256), 0, st, (const F2*)mill, k, count, digits(),
                         gt_out, expect, valid, ok);
    }
    ZK_PAIR_HIP(hipGetLastError());
    return ZK_OK;
  }

 public:
  int multi_pairing(IEngine* e, const void* p_d, const void* q_d, size_t k, size_t count, void* gt_out_d,
                    hipStream_t st) override {
    if (int rc = e->check_wedged()) return rc;
    if (!count) return ZK_OK;
    if (!p_d || !q_d || !gt_out_d) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (!k || k > (1u << 20) || count > ((size_t)1 << 40) / k) return e->fail(ZK_ERR_BAD_INPUT, "zk_multi_pairing: bad k or count");
    Workspace& ws = workspace(e->device);
    std::lock_guard<std::mutex> g(ws.mu);
    ZK_PAIR_HIP(ws.mill.ensure(count * k * 6 * sizeof(F2)));
    if (int rc = launch(e, p_d, q_d, k, count, (F2*)ws.mill.p, (F2*)gt_out_d, nullptr, nullptr, nullptr, st)) return rc;
    return wait(e, st, "zk_multi_pairing");        // (the Miller values are the next call's from here on)
  }

  int fq12_selftest(IEngine* e, int op, const void* a_d, const void* b_d, size_t len, void* out_d, hipStream_t st) override {
    if (int rc = e->check_wedged()) return rc;
    if (!len) return ZK_OK;
    if (op < 0 || op > 8) return e->fail(ZK_ERR_BAD_INPUT, "zk_fq12_selftest: op is 0..8");
    if (!a_d || !out_d || ((op == 0 || op == 8) && !b_d)) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
    hipLaunchKernelGGL(pairing_fq12_selftest_kernel<PP>, dim3(blocks(len)), dim3(256), 0, st, op, (const F2*)a_d, (const F2*)b_d,
                       len, (F2*)out_d);
    ZK_PAIR_HIP(hipGetLastError());
    return wait(e, st, "zk_fq12_selftest");
  }

  int vk_prepare(IEngine* e, const void* alpha_g1, const void* beta_g2, const void* gamma_g2, const void* delta_g2,
                 const void* gamma_abc_g1, size_t n_abc, zk_vk* vk) override {
    if (int rc = e->check_wedged()) return rc;
    if (!alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (!n_abc) return e->fail(ZK_ERR_BAD_INPUT, "malformed verifying key");
    vk->curve = CURVE;
    vk->device = e->device;
    vk->n_abc = n_abc;
    auto neg = [](const void* p) {
      Affine<F2> a;
      memcpy(&a, p, sizeof(a));
      if (!a.is_identity()) a.y = a.y.neg();
      return a;
    };
    const Affine<F2> ng = neg(gamma_g2), nd = neg(delta_g2);
    ZK_PAIR_HIP(hipMalloc(&vk->abc_d, n_abc * sizeof(Affine<Fq>)));
    ZK_PAIR_HIP(hipMalloc(&vk->neg_gamma_d, sizeof(Affine<F2>)));
    ZK_PAIR_HIP(hipMalloc(&vk->neg_delta_d, sizeof(Affine<F2>)));
    ZK_PAIR_HIP(hipMalloc(&vk->alpha_beta_d, 6 * sizeof(F2)));
    ZK_PAIR_HIP(hipMemcpy(vk->abc_d, gamma_abc_g1, n_abc * sizeof(Affine<Fq>), hipMemcpyHostToDevice));
    if (n_abc > 1) {
      ZK_PAIR_HIP(hipMalloc(&vk->abc_table_d, (n_abc - 1) * FrP::BITS * sizeof(XYZZ<Fq>)));
      hipLaunchKernelGGL((pairing_abc_table_kernel<Fq, FrP::BITS>), dim3((unsigned)((n_abc - 1 + 63) / 64)), dim3(64), 0, nullptr,
                         (const Affine<Fq>*)vk->abc_d, n_abc - 1, (XYZZ<Fq>*)vk->abc_table_d);
      ZK_PAIR_HIP(hipGetLastError());
    }
    ZK_PAIR_HIP(hipMemcpy(vk->neg_gamma_d, &ng, sizeof(ng), hipMemcpyHostToDevice));
    ZK_PAIR_HIP(hipMemcpy(vk->neg_delta_d, &nd, sizeof(nd), hipMemcpyHostToDevice));
    // the batch check's part: alpha, beta, the doubling tables of abc[0] and alpha (rows 0, 1 of one table), the Fq12 one
    Affine<Fq> base[3];
    base[0] = Affine<Fq>{Fq::zero(), Fq::zero()};
    memcpy(&base[1], gamma_abc_g1, sizeof(Affine<Fq>));
    memcpy(&base[2], alpha_g1, sizeof(Affine<Fq>));
    F2 one[6];
    for (int i = 0; i < 6; i++) one[i] = i ? F2::zero() : F2::one();
    ZK_PAIR_HIP(hipMalloc(&vk->rlc_base_d, sizeof(base)));
    ZK_PAIR_HIP(hipMalloc(&vk->rlc_table_d, 2 * FrP::BITS * sizeof(XYZZ<Fq>)));
    ZK_PAIR_HIP(hipMalloc(&vk->beta_d, sizeof(Affine<F2>)));
    ZK_PAIR_HIP(hipMalloc(&vk->one_d, sizeof(one)));
    ZK_PAIR_HIP(hipMemcpy(vk->rlc_base_d, base, sizeof(base), hipMemcpyHostToDevice));
    ZK_PAIR_HIP(hipMemcpy(vk->beta_d, beta_g2, sizeof(Affine<F2>), hipMemcpyHostToDevice));
    ZK_PAIR_HIP(hipMemcpy(vk->one_d, one, sizeof(one), hipMemcpyHostToDevice));
    hipLaunchKernelGGL((pairing_abc_table_kernel<Fq, FrP::BITS>), dim3(1), dim3(64), 0, nullptr, (const Affine<Fq>*)vk->rlc_base_d,
                       (size_t)2, (XYZZ<Fq>*)vk->rlc_table_d);
    ZK_PAIR_HIP(hipGetLastError());
    const Affine<Fq>* alpha_d = (const Affine<Fq>*)vk->rlc_base_d + 2;
    return multi_pairing(e, alpha_d, vk->beta_d, 1, 1, vk->alpha_beta_d, nullptr);      // e(alpha, beta), once
  }

  int verify(IEngine* e, const zk_vk* vk, const void* proofs, const void* inputs, size_t n_inputs, size_t count, uint8_t* ok,
             hipStream_t st) override {
    if (int rc = e->check_wedged()) return rc;
    if (int rc = verify_args(e, vk, n_inputs, "zk_groth16_verify")) return rc;
    if (!count) return ZK_OK;
    if (!proofs || !ok || (n_inputs && !inputs)) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (count > ((size_t)1 << 30)) return e->fail(ZK_ERR_BAD_INPUT, "zk_groth16_verify: count too large");
    Workspace& ws = workspace(e->device);
    std::lock_guard<std::mutex> g(ws.mu);
    if (int rc = verify_ensure(e, ws, n_inputs, count)) return rc;
    ZK_PAIR_HIP(hipMemcpyAsync(ws.proofs.p, proofs, count * sizeof(Proof), hipMemcpyHostToDevice, st));
    if (n_inputs) ZK_PAIR_HIP(hipMemcpyAsync(ws.inputs.p, inputs, count * n_inputs * sizeof(Fr), hipMemcpyHostToDevice, st));
    return verify_run(e, vk, ws, n_inputs, count, nullptr, ok, st, "zk_groth16_verify");
  }

 private:
  using Proof = ProofAffine<Fq, F2>;
  static_assert(sizeof(Proof) == 8 * sizeof(Fq), "A | B | C is eight Fq");
  static constexpr bool ZCASH = CURVE == ZK_BLS12_381;          // the point encoding of the curve's arkworks crate
  static constexpr size_t PROOF_BYTES = 4 * PointCodec<Fq>::SIZE, INPUT_BYTES = 32;

  int verify_args(IEngine* e, const zk_vk* vk, size_t n_inputs, const char* what) {
    if (!vk || vk->curve != CURVE || vk->device != e->device)
      return e->fail(ZK_ERR_BAD_INPUT, std::string(what) + ": the verifying key was prepared for another context");
    if (n_inputs + 1 != vk->n_abc) return e->fail(ZK_ERR_BAD_INPUT, "malformed verifying key");
    return ZK_OK;
  }
  int verify_ensure(IEngine* e, Workspace& ws, size_t n_inputs, size_t count) {
    ZK_PAIR_HIP(ws.proofs.ensure(count * sizeof(Proof)));
    ZK_PAIR_HIP(ws.inputs.ensure(count * n_inputs * sizeof(Fr) + 1));
    ZK_PAIR_HIP(ws.P.ensure(3 * count * sizeof(Affine<Fq>)));
    ZK_PAIR_HIP(ws.Q.ensure(3 * count * sizeof(Affine<F2>)));
    ZK_PAIR_HIP(ws.mill.ensure(3 * count * 6 * sizeof(F2)));
    ZK_PAIR_HIP(ws.valid.ensure(count));
    ZK_PAIR_HIP(ws.ok.ensure(count));
    return ZK_OK;
  }
  // The verdict stages of zk_groth16_verify over the proofs and inputs staged in the workspace (held by the caller).  valid0
  // (device, one byte per proof; null from the host-pointer entry point) joins the validity bytes the prep kernel writes.
  int verify_run(IEngine* e, const zk_vk* vk, Workspace& ws, size_t n_inputs, size_t count, const uint8_t* valid0, uint8_t* ok,
                 hipStream_t st, const char* what) {
    hipLaunchKernelGGL((pairing_verify_prep_kernel<PP, FrP>), dim3((unsigned)count), dim3(64), 0, st,
                       (const Proof*)ws.proofs.p, (const Fr*)ws.inputs.p, n_inputs, (const Affine<Fq>*)vk->abc_d,
                       (const XYZZ<Fq>*)vk->abc_table_d,
                       (const Affine<F2>*)vk->neg_gamma_d, (const Affine<F2>*)vk->neg_delta_d, B1, count, (Affine<Fq>*)ws.P.p,
                       (Affine<F2>*)ws.Q.p, (uint8_t*)ws.valid.p);
    if (valid0) valid_and(e, (uint8_t*)ws.valid.p, valid0, count, st);
    int rc = launch(e, ws.P.p, ws.Q.p, 3, count, (F2*)ws.mill.p, nullptr, (const F2*)vk->alpha_beta_d, (const uint8_t*)ws.valid.p,
                    (uint8_t*)ws.ok.p, st);
    if (!rc) {
      hipError_t h = hipMemcpyAsync(ok, ws.ok.p, count, hipMemcpyDeviceToHost, st);
      if (h != hipSuccess) rc = e->hip_fail(h, (std::string(what) + ": copy of the verdicts").c_str());
    }
    const int wrc = wait(e, st, what);      // also on an error path: the workspace is handed on after it
    return rc ? rc : wrc;
  }
  static void valid_and(IEngine* e, uint8_t* valid, const uint8_t* valid0, size_t count, hipStream_t st) {
    ProfScope ps(e->prof, PROF_STAGE_VALID, st, (double)count);
    hipLaunchKernelGGL(verify_valid_and_kernel<PP>, dim3((unsigned)div256(count)), dim3(256), 0, st, valid, valid0, count);
  }

  static size_t div256(size_t n) { return (n + 255) / 256; }
  // the sum of in[0 .. n) (and the AND of vin[0 .. n)) by pairing_rlc_sum_kernel, 256 to 1 per launch and at least once;
  // a / b (va / vb) take the levels in turn: a holds div256(n) entries, b div256(div256(n))
  static const XYZZ<Fq>* tree_sum(IEngine* e, const XYZZ<Fq>* in, const uint8_t* vin, size_t n, XYZZ<Fq>* a, XYZZ<Fq>* b, uint8_t* va,
                                  uint8_t* vb, const uint8_t** vout, hipStream_t st) {
    ProfScope ps(e->prof, PROF_RLC_SUM, st, (double)n);
    for (;;) {
      const size_t m = div256(n);
      hipLaunchKernelGGL(pairing_rlc_sum_kernel<Fq>, dim3((unsigned)m), dim3(256), 0, st, in, vin, n, a, va);
      in = a, vin = va, n = m;
      if (n == 1) break;
      std::swap(a, b);
      std::swap(va, vb);
    }
    if (vout) *vout = vin;
    return in;
  }

 private:
  // what both batch entry points do before they stage: the argument errors, the empty batch, the randomizer key
  // (returns 1 when the call is already answered)
  int verify_all_begin(IEngine* e, const zk_vk* vk, const void* proofs, const void* inputs, size_t n_inputs, size_t count,
                       const uint8_t* seed, int* all_ok, void* gt_out, const char* what, RlcKey* key, int* rc_out) {
    *rc_out = ZK_OK;
    if (int rc = e->check_wedged()) return *rc_out = rc, 1;
    if (int rc = verify_args(e, vk, n_inputs, what)) return *rc_out = rc, 1;
    if (!all_ok) return *rc_out = e->fail(ZK_ERR_BAD_INPUT, "null pointer"), 1;
    if (!count) {
      *all_ok = 1;
      if (gt_out) {
        F2 one[6];
        for (int i = 0; i < 6; i++) one[i] = i ? F2::zero() : F2::one();
        memcpy(gt_out, one, sizeof(one));
      }
      return 1;
    }
    if (!proofs || (n_inputs && !inputs)) return *rc_out = e->fail(ZK_ERR_BAD_INPUT, "null pointer"), 1;
    if (count > ((size_t)1 << 30)) return *rc_out = e->fail(ZK_ERR_BAD_INPUT, std::string(what) + ": count too large"), 1;
    uint8_t drawn[32];
    if (!seed) {
      FILE* f = fopen("/dev/urandom", "rb");
      const size_t got = f ? fread(drawn, 1, sizeof(drawn), f) : 0;
      if (f) fclose(f);
      if (got != sizeof(drawn))
        return *rc_out = e->fail(ZK_ERR_GENERIC, "cannot read /dev/urandom for the batch check's randomizers"), 1;
      seed = drawn;
    }
    *key = rlc_key(seed);
    return 0;
  }
  struct RlcSizes {
    size_t n_abc, npairs, c1, c2, gblk, g1, g2;
    GtFoldPlan plan;
  };
  static RlcSizes rlc_sizes(const zk_vk* vk, size_t count) {
    RlcSizes z;
    z.n_abc = vk->n_abc, z.npairs = count + 3;
    z.plan = gt_fold_plan(z.npairs);
    // r_i C_i | the two levels of their sum | the gamma kernel's partial sums (+ s alpha) | the two levels of theirs
    z.c1 = div256(count), z.c2 = div256(z.c1), z.gblk = (z.n_abc + RLC_GAMMA_ROWS - 1) / RLC_GAMMA_ROWS, z.g1 = div256(z.gblk),
    z.g2 = div256(z.g1);
    return z;
  }
  int verify_all_ensure(IEngine* e, Workspace& ws, const RlcSizes& z, size_t n_inputs, size_t count) {
    using Pt = XYZZ<Fq>;
    ZK_PAIR_HIP(ws.proofs.ensure(count * sizeof(Proof)));
    ZK_PAIR_HIP(ws.inputs.ensure(count * n_inputs * sizeof(Fr) + 1));
    ZK_PAIR_HIP(ws.P.ensure(z.npairs * sizeof(Affine<Fq>)));
    ZK_PAIR_HIP(ws.Q.ensure(z.npairs * sizeof(Affine<F2>)));
    ZK_PAIR_HIP(ws.mill.ensure(z.npairs * 6 * sizeof(F2)));
    ZK_PAIR_HIP(ws.rlc_pts.ensure((count + z.c1 + z.c2 + z.gblk + 1 + z.g1 + z.g2) * sizeof(Pt)));
    ZK_PAIR_HIP(ws.rlc_fr.ensure((count + z.n_abc) * sizeof(Fr)));
    ZK_PAIR_HIP(ws.rlc_bytes.ensure(count + z.c1 + z.c2 + 2));
    ZK_PAIR_HIP(ws.rlc_gt.ensure((z.plan.G + 1) * 6 * sizeof(F2)));
    return ZK_OK;
  }
  // The verdict stages of zk_groth16_verify_all over the proofs and inputs staged in the workspace (held by the caller); rc is
  // what the staging left (nothing is launched after an error, the wait is made all the same).  valid0 (device, one byte per
  // proof; null from the host-pointer entry point) joins the validity bytes before the tree sum folds them.
  int verify_all_run(IEngine* e, const zk_vk* vk, Workspace& ws, const RlcSizes& z, const RlcKey& key, size_t n_inputs, size_t count,
                     const uint8_t* valid0, int rc, int* all_ok, void* gt_out, hipStream_t st, const char* what) {
    using Pt = XYZZ<Fq>;
    const size_t n_abc = z.n_abc, npairs = z.npairs, c1 = z.c1, c2 = z.c2, gblk = z.gblk, g1 = z.g1;
    const GtFoldPlan& plan = z.plan;
    Pt *cx = (Pt*)ws.rlc_pts.p, *ca = cx + count, *cb = ca + c1, *gpart = cb + c2, *ga = gpart + gblk + 1, *gb = ga + g1;
    Fr *rfr = (Fr*)ws.rlc_fr.p, *sdot = rfr + count;
    uint8_t *valid = (uint8_t*)ws.rlc_bytes.p, *va = valid + count, *vb = va + c1, *all_valid = vb + c2, *okd = all_valid + 1;
    F2 *gfold = (F2*)ws.rlc_gt.p, *gt_d = gfold + plan.G * 6;
    Affine<Fq>* P = (Affine<Fq>*)ws.P.p;
    Affine<F2>* Q = (Affine<F2>*)ws.Q.p;
    const std::string w(what);
    auto step = [&](hipError_t h, const char* part) {
      if (!rc && h != hipSuccess) rc = e->hip_fail(h, (w + part).c_str());
    };
    if (!rc) {
      {
        ProfScope ps(e->prof, PROF_RLC_SCALE, st, (double)count);
        hipLaunchKernelGGL((pairing_rlc_scale_kernel<PP, FrP>), dim3((unsigned)div256(2 * count)), dim3(256), 0, st,
                           (const Proof*)ws.proofs.p, key, B1, count, P, Q, cx, rfr, valid);
      }
      if (valid0) valid_and(e, valid, valid0, count, st);
      {
        ProfScope ps(e->prof, PROF_RLC_DOT, st, (double)n_abc);
        hipLaunchKernelGGL(pairing_rlc_dot_kernel<FrP>, dim3((unsigned)n_abc), dim3(256), 0, st, (const Fr*)rfr,
                           (const Fr*)ws.inputs.p, n_inputs, count, sdot);
      }
      const uint8_t* vall = nullptr;
      const Pt* p_delta = tree_sum(e, cx, valid, count, ca, cb, va, vb, &vall, st);
      {
        ProfScope ps(e->prof, PROF_RLC_GAMMA, st, (double)n_abc + 1);
        hipLaunchKernelGGL((pairing_rlc_gamma_kernel<Fq, FrP>), dim3((unsigned)gblk + 1), dim3(64), 0, st, (const Fr*)sdot, n_abc,
                           (const Pt*)vk->abc_table_d, (const Pt*)vk->rlc_table_d, gpart);
      }
      const Pt* p_gamma = gblk == 1 ? gpart : tree_sum(e, gpart, nullptr, gblk, ga, gb, nullptr, nullptr, nullptr, st);
      {
        ProfScope ps(e->prof, PROF_RLC_FINISH, st, 3.0);
        hipLaunchKernelGGL((pairing_rlc_finish_kernel<Fq, F2>), dim3(1), dim3(64), 0, st, p_gamma, p_delta, (const Pt*)(gpart + gblk),
                           vall, (const Affine<F2>*)vk->neg_gamma_d, (const Affine<F2>*)vk->neg_delta_d,
                           (const Affine<F2>*)vk->beta_d, count, P, Q, all_valid);
      }
      {
        ProfScope ps(e->prof, PROF_MILLER, st, (double)npairs);
        hipLaunchKernelGGL(pairing_miller_kernel<PP>, dim3(blocks(npairs)), dim3(256), 0, st, (const Affine<Fq>*)P,
                           (const Affine<F2>*)Q, npairs, (F2*)ws.mill.p);
      }
      {
        ProfScope ps(e->prof, PROF_GT_FOLD, st, (double)npairs);
        hipLaunchKernelGGL(pairing_gt_fold_kernel<PP>, dim3(blocks(plan.G)), dim3(256), 0, st, (const F2*)ws.mill.p, npairs, plan.G,
                           plan.len, gfold);
      }
      {
        ProfScope ps(e->prof, PROF_FINAL_EXP, st, 1.0);
        hipLaunchKernelGGL(pairing_final_exp_kernel<PP>, dim3(1), dim3(256), 0, st, (const F2*)gfold, plan.G, (size_t)1, digits(),
                           gt_d, (const F2*)vk->one_d, (const uint8_t*)all_valid, okd);
      }
      step(hipGetLastError(), ": launch");
      step(hipMemcpyAsync(&ws.host_ok, okd, 1, hipMemcpyDeviceToHost, st), ": copy of the verdict");
      if (gt_out) step(hipMemcpyAsync(ws.host_gt, gt_d, sizeof(ws.host_gt), hipMemcpyDeviceToHost, st), ": copy of the value");
    }
    const int wrc = wait(e, st, what);      // also on an error path: the workspace is handed on after it
    if (rc || wrc) return rc ? rc : wrc;
    *all_ok = ws.host_ok != 0;
    if (gt_out) memcpy(gt_out, ws.host_gt, sizeof(ws.host_gt));
    return ZK_OK;
  }

  // Staging of the bytes verifiers: the wire bytes go up in one buffer (proofs, then inputs), two launches leave the
  // ProofAffine array, the Montgomery inputs and one validity byte per proof in the workspace.  Returns the validity bytes.
  int stage_ensure(IEngine* e, Workspace& ws, size_t n_inputs, size_t count) {
    ZK_PAIR_HIP(ws.wire.ensure(count * (PROOF_BYTES + n_inputs * INPUT_BYTES)));
    ZK_PAIR_HIP(ws.stage_ok.ensure(4 * count));
    return ZK_OK;
  }
  const uint8_t* stage(IEngine* e, Workspace& ws, const void* proof_bytes, const void* input_bytes, size_t n_inputs, size_t count,
                       hipStream_t st, const char* what, int* rc) {
    uint8_t *wire = (uint8_t*)ws.wire.p, *wire_in = wire + count * PROOF_BYTES;
    uint8_t *pok = (uint8_t*)ws.stage_ok.p, *valid0 = pok + 3 * count;
    const std::string w(what);
    auto step = [&](hipError_t h, const char* part) {
      if (!*rc && h != hipSuccess) *rc = e->hip_fail(h, (w + part).c_str());
    };
    step(hipMemcpyAsync(wire, proof_bytes, count * PROOF_BYTES, hipMemcpyHostToDevice, st), ": copy of the proof bytes");
    if (n_inputs)
      step(hipMemcpyAsync(wire_in, input_bytes, count * n_inputs * INPUT_BYTES, hipMemcpyHostToDevice, st), ": copy of the input bytes");
    if (*rc) return valid0;
    const size_t nb = (count + 63) / 64 * 64;
    {
      ProfScope ps(e->prof, PROF_STAGE_POINTS, st, (double)count);
      hipLaunchKernelGGL(verify_stage_points_kernel<PP>, dim3((unsigned)((nb + 2 * count + 63) / 64)), dim3(64), 0, st,
                         (const uint8_t*)wire, count, nb, B1, ZCASH ? 1 : 0, (Proof*)ws.proofs.p, pok);
    }
    {
      ProfScope ps(e->prof, PROF_STAGE_INPUTS, st, (double)count);
      hipLaunchKernelGGL(verify_stage_inputs_kernel<FrP>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, (const uint8_t*)wire_in,
                         n_inputs, count, (const uint8_t*)pok, (Fr*)ws.inputs.p, valid0);
    }
    return valid0;
  }

 public:
  int verify_all(IEngine* e, const zk_vk* vk, const void* proofs, const void* inputs, size_t n_inputs, size_t count,
                 const uint8_t* seed, int* all_ok, void* gt_out, hipStream_t st) override {
    const char* what = "zk_groth16_verify_all";
    RlcKey key;
    int rc = ZK_OK;
    if (verify_all_begin(e, vk, proofs, inputs, n_inputs, count, seed, all_ok, gt_out, what, &key, &rc)) return rc;
    const RlcSizes z = rlc_sizes(vk, count);
    Workspace& ws = workspace(e->device);
    std::lock_guard<std::mutex> g(ws.mu);
    if (int erc = verify_all_ensure(e, ws, z, n_inputs, count)) return erc;
    auto step = [&](hipError_t h, const char* part) {
      if (!rc && h != hipSuccess) rc = e->hip_fail(h, part);
    };
    step(hipMemcpyAsync(ws.proofs.p, proofs, count * sizeof(Proof), hipMemcpyHostToDevice, st), "zk_groth16_verify_all: copy of the proofs");
    if (n_inputs)
      step(hipMemcpyAsync(ws.inputs.p, inputs, count * n_inputs * sizeof(Fr), hipMemcpyHostToDevice, st),
           "zk_groth16_verify_all: copy of the public inputs");
    return verify_all_run(e, vk, ws, z, key, n_inputs, count, nullptr, rc, all_ok, gt_out, st, what);
  }

  // ---- subgroup membership, checked decompression, the verifiers from wire bytes
  int points_subgroup_check(IEngine* e, int group, const void* affine_d, size_t len, uint8_t* ok_d, hipStream_t st) override {
    if (int rc = e->check_wedged()) return rc;
    if (group != ZK_G1 && group != ZK_G2) return e->fail(ZK_ERR_BAD_INPUT, "zk_points_subgroup_check: group is ZK_G1 or ZK_G2");
    if (!len) return ZK_OK;
    if (!affine_d || !ok_d) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (len > ((size_t)1 << 36)) return e->fail(ZK_ERR_BAD_INPUT, "zk_points_subgroup_check: len too large");
    const dim3 grid((unsigned)((len + 63) / 64));
    {
      ProfScope ps(e->prof, group == ZK_G2 ? PROF_SUBGROUP_G2 : PROF_SUBGROUP_G1, st, (double)len);
      if (group == ZK_G2)
        hipLaunchKernelGGL((points_subgroup_check_kernel<PP, true>), grid, dim3(64), 0, st, (const Affine<F2>*)affine_d, len, B1, ok_d);
      else
        hipLaunchKernelGGL((points_subgroup_check_kernel<PP, false>), grid, dim3(64), 0, st, (const Affine<Fq>*)affine_d, len, B1, ok_d);
    }
    ZK_PAIR_HIP(hipGetLastError());
    return wait(e, st, "zk_points_subgroup_check");
  }
  int points_decompress_checked(IEngine* e, int group, const void* bytes_d, size_t len, void* out_affine_d, uint8_t* ok_d,
                                hipStream_t st) override {
    if (int rc = e->check_wedged()) return rc;
    if (group != ZK_G1 && group != ZK_G2) return e->fail(ZK_ERR_BAD_INPUT, "zk_points_decompress_checked: group is ZK_G1 or ZK_G2");
    if (!len) return ZK_OK;
    if (!bytes_d || !out_affine_d || !ok_d) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (len > ((size_t)1 << 36)) return e->fail(ZK_ERR_BAD_INPUT, "zk_points_decompress_checked: len too large");
    const dim3 grid((unsigned)((len + 63) / 64));
    {
      ProfScope ps(e->prof, PROF_DECOMPRESS_CHECKED, st, (double)len);
      if (group == ZK_G2)
        hipLaunchKernelGGL((points_decompress_checked_kernel<PP, true>), grid, dim3(64), 0, st, (const uint8_t*)bytes_d, len, B1,
                           ZCASH ? 1 : 0, (Affine<F2>*)out_affine_d, ok_d);
      else
        hipLaunchKernelGGL((points_decompress_checked_kernel<PP, false>), grid, dim3(64), 0, st, (const uint8_t*)bytes_d, len, B1,
                           ZCASH ? 1 : 0, (Affine<Fq>*)out_affine_d, ok_d);
    }
    ZK_PAIR_HIP(hipGetLastError());
    return wait(e, st, "zk_points_decompress_checked");
  }
  int verify_bytes(IEngine* e, const zk_vk* vk, const void* proof_bytes, const void* input_bytes, size_t n_inputs, size_t count,
                   uint8_t* ok, hipStream_t st) override {
    const char* what = "zk_groth16_verify_bytes";
    if (int rc = e->check_wedged()) return rc;
    if (int rc = verify_args(e, vk, n_inputs, what)) return rc;
    if (!count) return ZK_OK;
    if (!proof_bytes || !ok || (n_inputs && !input_bytes)) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (count > ((size_t)1 << 30)) return e->fail(ZK_ERR_BAD_INPUT, "zk_groth16_verify_bytes: count too large");
    Workspace& ws = workspace(e->device);
    std::lock_guard<std::mutex> g(ws.mu);
    if (int rc = verify_ensure(e, ws, n_inputs, count)) return rc;
    if (int rc = stage_ensure(e, ws, n_inputs, count)) return rc;
    int rc = ZK_OK;
    const uint8_t* valid0 = stage(e, ws, proof_bytes, input_bytes, n_inputs, count, st, what, &rc);
    if (rc) {
      (void)wait(e, st, what);      // the workspace is handed on after it
      return rc;
    }
    return verify_run(e, vk, ws, n_inputs, count, valid0, ok, st, what);
  }
  int verify_all_bytes(IEngine* e, const zk_vk* vk, const void* proof_bytes, const void* input_bytes, size_t n_inputs, size_t count,
                       const uint8_t* seed, int* all_ok, void* gt_out, hipStream_t st) override {
    const char* what = "zk_groth16_verify_all_bytes";
    RlcKey key;
    int rc = ZK_OK;
    if (verify_all_begin(e, vk, proof_bytes, input_bytes, n_inputs, count, seed, all_ok, gt_out, what, &key, &rc)) return rc;
    const RlcSizes z = rlc_sizes(vk, count);
    Workspace& ws = workspace(e->device);
    std::lock_guard<std::mutex> g(ws.mu);
    if (int erc = verify_all_ensure(e, ws, z, n_inputs, count)) return erc;
    if (int erc = stage_ensure(e, ws, n_inputs, count)) return erc;
    const uint8_t* valid0 = stage(e, ws, proof_bytes, input_bytes, n_inputs, count, st, what, &rc);
    return verify_all_run(e, vk, ws, z, key, n_inputs, count, valid0, rc, all_ok, gt_out, st, what);
  }
};

}  // namespace zk
