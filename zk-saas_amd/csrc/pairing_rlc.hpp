// Kernels of zk_groth16_verify_all: one randomized pairing check for a whole batch of Groth16 proofs.
//
// For proofs i < count and 128-bit randomizers r_i != 0 (pairing_rlc_plan.hpp) the batch is accepted when
//   prod_i e(r_i A_i, B_i) * e(P_gamma, -gamma) * e(P_delta, -delta) * e(-s alpha, beta) = 1,
//   s = sum r_i,  s_t = sum_i r_i x_{i,t} (mod r),  P_gamma = s abc[0] + sum_t s_t abc[t + 1],  P_delta = sum_i r_i C_i:
// count + 3 Miller loops and ONE final exponentiation, where zk_groth16_verify pays three and one per proof.  The launches:
//   pairing_rlc_scale_kernel   per proof: the validity test, r_i A_i (affine, pair i), r_i C_i (XYZZ), r_i as an Fr element
//   pairing_rlc_dot_kernel     s and s_t: one workgroup per sum
//   pairing_rlc_sum_kernel     P_delta (and the AND of the validity bytes): 256 points per workgroup, as often as it takes
//   pairing_rlc_gamma_kernel   the table entries 2^k abc[t] of the set bits of s_t: one wave per RLC_GAMMA_ROWS rows, and one
//                              more for s alpha; the partial sums go through pairing_rlc_sum_kernel again
//   pairing_rlc_finish_kernel  the three key pairs count .. count + 2
//   pairing_miller_kernel      unchanged
//   pairing_gt_fold_kernel     G = ceil(sqrt(count + 3)) lane groups multiply a range of Miller values each (GtFoldPlan);
//                              pairing_final_exp_kernel then runs with k = G, count = 1 and expect = 1
// No chain of dependent operations grows with count faster than its square root, but the strided Fr sums of the dot kernel
// (count / 256 additions per thread).
#pragma once
#include "pairing_rlc_plan.hpp"

namespace zk {

constexpr int RLC_GAMMA_ROWS = 8;      // table rows (key points) per wave of pairing_rlc_gamma_kernel

// the validity test of pairing_verify_prep_kernel: canonical coordinates, on the curve (the identity counts as on it)
template <class Fq>
__device__ bool rlc_on_g1(const Affine<Fq>& p, int b1) {
  if (!p.x.is_canonical() || !p.y.is_canonical()) return false;
  return p.is_identity() || Fq::mul_ni(p.y, p.y) == Fq::mul_ni(Fq::mul_ni(p.x, p.x), p.x) + Fq::from_u64((uint64_t)b1);
}
template <class PP>
__device__ bool rlc_on_g2(const Affine<typename Tower<PP>::F2>& p) {
  using T = Tower<PP>;
  if (!p.x.c0.is_canonical() || !p.x.c1.is_canonical() || !p.y.c0.is_canonical() || !p.y.c1.is_canonical()) return false;
  return p.is_identity() || p.y.sqr() == p.x.sqr() * p.x + T::f2_const(PP::TWIST_B);
}

// Two lanes per proof: the even one tests the proof and scales A, the odd one scales C.  A proof that fails the test has its
// pair replaced by identities and contributes the identity to P_delta: nothing is computed from a point that is not on its
// curve, and valid[i] = 0 rejects the batch whatever the pairings give.
template <class PP, class FrP>
__global__ __launch_bounds__(256) void pairing_rlc_scale_kernel(
    const ProofAffine<typename Tower<PP>::Fq, typename Tower<PP>::F2>* __restrict__ proofs, RlcKey key, int b1, size_t count,
    Affine<typename Tower<PP>::Fq>* __restrict__ P, Affine<typename Tower<PP>::F2>* __restrict__ Q,
    XYZZ<typename Tower<PP>::Fq>* __restrict__ cx, Fp<FrP>* __restrict__ r_out, uint8_t* __restrict__ valid) {
  using Fq = typename Tower<PP>::Fq;
  using F2 = typename Tower<PP>::F2;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = idx >> 1;
  if (i >= count) return;
  const bool is_c = (idx & 1) != 0;
  uint32_t r[4];
  rlc_randomizer(key, (uint64_t)i, r);
  const Affine<Fq> pt = is_c ? proofs[i].C : proofs[i].A;
  bool ok = rlc_on_g1(pt, b1);
  if (!is_c) {
    const Affine<F2> B = proofs[i].B;
    ok = ok && rlc_on_g2<PP>(B) && rlc_on_g1(proofs[i].C, b1);
    valid[i] = (uint8_t)ok;
    Q[i] = ok ? B : Affine<F2>{F2::zero(), F2::zero()};
    Fp<FrP> rf = Fp<FrP>::zero();
#pragma unroll
    for (int j = 0; j < 4; j++) rf.v[j] = r[j];
    r_out[i] = rf.to_mont();
  }
  const XYZZ<Fq> base = ok ? XYZZ<Fq>::from_affine(pt) : XYZZ<Fq>::identity();
  XYZZ<Fq> acc = XYZZ<Fq>::identity();
#pragma unroll 1
  for (int b = 127; b >= 0; b--) {
    acc = xyzz_dbl_ni(acc);
    if ((r[b >> 5] >> (b & 31)) & 1u) acc = xyzz_add_ni(acc, base);
  }
  if (is_c) cx[i] = acc;
  else P[i] = xyzz_to_affine(acc);
}

// out[0] = sum_i r_i, out[t + 1] = sum_i r_i x_{i,t}, as canonical integers (the gamma kernel reads their bits); workgroup b
// computes out[b]
template <class FrP>
__global__ __launch_bounds__(256) void pairing_rlc_dot_kernel(const Fp<FrP>* __restrict__ r, const Fp<FrP>* __restrict__ inputs,
                                                              size_t n_inputs, size_t count, Fp<FrP>* __restrict__ out) {
  using Fr = Fp<FrP>;
  __shared__ Fr sh[256];
  const size_t b = blockIdx.x;
  const unsigned tid = threadIdx.x;
  Fr acc = Fr::zero();
#pragma unroll 1
  for (size_t i = tid; i < count; i += 256) acc = acc + (b == 0 ? r[i] : Fr::mul_ni(r[i], inputs[i * n_inputs + (b - 1)]));
  sh[tid] = acc;
  __syncthreads();
#pragma unroll 1
  for (unsigned off = 128; off >= 1; off >>= 1) {
    if (tid < off) sh[tid] = sh[tid] + sh[tid + off];
    __syncthreads();
  }
  if (tid == 0) out[b] = sh[0].from_mont();
}

// the sum of a wave's 64 points in lane 0: six exchange rounds, made with the wave converged (the additions may diverge)
template <class Fq>
__device__ XYZZ<Fq> rlc_wave_sum(XYZZ<Fq> acc, int lane) {
#pragma unroll 1
  for (int off = 32; off >= 1; off >>= 1) {
    const XYZZ<Fq> other = xyzz_from_lane(acc, (lane + off) & 63);
    acc = xyzz_add_ni(acc, other);                // (lanes >= off compute sums nobody reads)
  }
  return acc;
}

// out[b] = in[256 b] + ... + in[256 b + 255] (short at the end), vout[b] = the AND of the same range of vin (either may be null)
template <class Fq>
__global__ __launch_bounds__(256) void pairing_rlc_sum_kernel(const XYZZ<Fq>* __restrict__ in, const uint8_t* __restrict__ vin,
                                                              size_t n, XYZZ<Fq>* __restrict__ out, uint8_t* __restrict__ vout) {
  __shared__ XYZZ<Fq> sh[4];
  const unsigned tid = threadIdx.x;
  const int lane = (int)(tid & 63u);
  const size_t idx = (size_t)blockIdx.x * 256 + tid;
  const XYZZ<Fq> mine = idx < n ? in[idx] : XYZZ<Fq>::identity();
  const int v = (vin && idx < n) ? vin[idx] != 0 : 1;
  const XYZZ<Fq> acc = rlc_wave_sum(mine, lane);
  if (lane == 0) sh[tid >> 6] = acc;
  const int all = __syncthreads_and(v);
  if (tid != 0) return;
  out[blockIdx.x] = xyzz_add_ni(xyzz_add_ni(sh[0], sh[1]), xyzz_add_ni(sh[2], sh[3]));
  if (vout) vout[blockIdx.x] = (uint8_t)(all != 0);
}

// Workgroup b < gridDim.x - 1 (one wave): out[b] = sum of s_t abc[t] over its RLC_GAMMA_ROWS rows t, with s_0 = s; the last
// workgroup: out[b] = s alpha.  Lane l sums the table entries of the set bits l, l + 64, ... of every scalar, as
// pairing_verify_prep_kernel does.  table = the key's [n_abc - 1][BITS] rows of abc[1..]; own = [2][BITS]: abc[0], alpha.
template <class Fq, class FrP>
__global__ __launch_bounds__(64) void pairing_rlc_gamma_kernel(const Fp<FrP>* __restrict__ sdot, size_t n_abc,
                                                               const XYZZ<Fq>* __restrict__ table, const XYZZ<Fq>* __restrict__ own,
                                                               XYZZ<Fq>* __restrict__ out) {
  constexpr int BITS = FrP::BITS;
  const size_t blk = blockIdx.x, nblk = gridDim.x - 1;
  const int lane = (int)threadIdx.x;
  const size_t t0 = blk == nblk ? 0 : blk * RLC_GAMMA_ROWS;
  const size_t t1 = blk == nblk ? 1 : (t0 + RLC_GAMMA_ROWS < n_abc ? t0 + RLC_GAMMA_ROWS : n_abc);
  XYZZ<Fq> acc = XYZZ<Fq>::identity();
#pragma unroll 1
  for (size_t t = t0; t < t1; t++) {              // (uniform)
    const Fp<FrP> x = sdot[t];
    const XYZZ<Fq>* row = blk == nblk ? own + BITS : t == 0 ? own : table + (t - 1) * BITS;
#pragma unroll 1
    for (int k = lane; k < BITS; k += 64)
      if ((x.v[k >> 5] >> (k & 31)) & 1u) acc = xyzz_add_ni(acc, row[k]);
  }
  acc = rlc_wave_sum(acc, lane);
  if (lane == 0) out[blk] = acc;
}

// pairs count .. count + 2: (P_gamma, -gamma), (P_delta, -delta), (-s alpha, beta), one lane each; the folded validity byte
template <class Fq, class F2>
__global__ __launch_bounds__(64) void pairing_rlc_finish_kernel(const XYZZ<Fq>* __restrict__ p_gamma, const XYZZ<Fq>* __restrict__ p_delta,
                                                                const XYZZ<Fq>* __restrict__ s_alpha, const uint8_t* __restrict__ vall,
                                                                const Affine<F2>* __restrict__ neg_gamma,
                                                                const Affine<F2>* __restrict__ neg_delta,
                                                                const Affine<F2>* __restrict__ beta, size_t count,
                                                                Affine<Fq>* __restrict__ P, Affine<F2>* __restrict__ Q,
                                                                uint8_t* __restrict__ all_valid) {
  const int lane = (int)threadIdx.x;
  if (lane > 2) return;
  const XYZZ<Fq> p = lane == 0 ? *p_gamma : lane == 1 ? *p_delta : s_alpha->neg();
  P[count + lane] = xyzz_to_affine(p);
  Q[count + lane] = lane == 0 ? *neg_gamma : lane == 1 ? *neg_delta : *beta;
  if (lane == 0) *all_valid = *vall;
}

// out[g] = prod of mill[g len .. min(n, (g + 1) len)), g < G (GtFoldPlan); 1 for an empty range.  Every lane group runs
// `len` rounds, a round past its range keeps the value, so the exchanges of L.mul are made with the wave converged.
template <class PP>
__global__ __launch_bounds__(256) void pairing_gt_fold_kernel(const typename Tower<PP>::F2* __restrict__ mill, size_t n, size_t G,
                                                              size_t len, typename Tower<PP>::F2* __restrict__ out) {
  using L12 = Lane12<PP>;
  using F2 = typename Tower<PP>::F2;
  const L12 L = L12::here();
  size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / PAIRING_GW;
  const bool live = g < G;
  if (!live) g = G - 1;
  const size_t lo = g * len < n ? g * len : n, hi = (g + 1) * len < n ? (g + 1) * len : n;
  F2 f = L.one();
#pragma unroll 1
  for (size_t s = 0; s < len; s++) {
    const size_t t = lo + s;
    const F2 m = L.mul(f, L.load(mill + (t < n ? t : n - 1) * 6));
    f = L12::sel(t < hi, m, f);
  }
  if (live) L.store(out + g * 6, f);
}

}  // namespace zk
