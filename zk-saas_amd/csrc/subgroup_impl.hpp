// Kernels of the checked entry points (subgroup.hpp is the arithmetic): zk_points_subgroup_check,
// zk_points_decompress_checked and the staging of zk_groth16_verify_bytes / zk_groth16_verify_all_bytes.  Compiled per
// curve with the verifier (pairing_<curve>.hip), apart from the prover's translation units.
//
// One lane per point; a lane holds one XYZZ point and the affine input.  The chains of subgroup.hpp run over compile-time
// constants through the out-of-line point steps, so every lane of a wave walks the same 63 / 64 (twice that for G1 of
// BLS12-381) doublings whatever its point is; a lane whose point already failed an earlier test leaves early.
#pragma once
#include <type_traits>

#include "points.hpp"
#include "subgroup.hpp"

namespace zk {

template <class PP, bool G2>
using SubgroupFld = typename std::conditional<G2, typename Tower<PP>::F2, typename Tower<PP>::Fq>::type;

template <class PP, bool G2>
__device__ bool subgroup_check_point(const Affine<SubgroupFld<PP, G2>>& p, int b1) {
  if constexpr (G2) return Subgroup<PP>::g2_check(p);
  else return Subgroup<PP>::g1_check(p, b1);
}
// decode + subgroup test of one element, as arkworks' deserialize_compressed (Validate::Yes): *out is (0,0) for an invalid
// encoding and the decoded point otherwise, also when it is outside the subgroup
template <class PP, bool G2>
__device__ bool decode_checked_point(const uint8_t* __restrict__ p, int b1, int zcash, Affine<SubgroupFld<PP, G2>>* out) {
  using Fld = SubgroupFld<PP, G2>;
  using S = Subgroup<PP>;
  Fld b;
  if constexpr (G2) b = S::twist_b();
  else b = Fld::from_u64((uint64_t)b1);
  bool ok;
  *out = point_decode(p, b, zcash, NoTs{}, &ok);
  if (ok && !out->is_identity()) {
    if constexpr (G2) ok = S::g2_in_subgroup(*out);
    else ok = S::g1_in_subgroup(*out);
  }
  return ok;
}

template <class PP, bool G2>
__global__ __launch_bounds__(64) void points_subgroup_check_kernel(const Affine<SubgroupFld<PP, G2>>* __restrict__ pts, size_t len,
                                                                  int b1, uint8_t* __restrict__ ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  ok[i] = (uint8_t)subgroup_check_point<PP, G2>(load_elem(pts + i), b1);
}

template <class PP, bool G2>
__global__ __launch_bounds__(64) void points_decompress_checked_kernel(const uint8_t* __restrict__ bytes, size_t len, int b1, int zcash,
                                                                      Affine<SubgroupFld<PP, G2>>* __restrict__ out,
                                                                      uint8_t* __restrict__ ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  Affine<SubgroupFld<PP, G2>> r;
  const bool good = decode_checked_point<PP, G2>(bytes + i * PointCodec<SubgroupFld<PP, G2>>::SIZE, b1, zcash, &r);
  store_elem(out + i, r);
  ok[i] = (uint8_t)good;
}

// Staging of the bytes verifiers, first launch: `Proof::serialize_compressed` bytes [count][A | B | C] -> ProofAffine[count]
// and three verdict bytes per proof.  The first nb = count rounded up to whole waves lanes take the B of a proof each, the
// 2 count lanes after them A (even) and C (odd): a wave is all G2 or all G1.
template <class PP>
__global__ __launch_bounds__(64) void verify_stage_points_kernel(
    const uint8_t* __restrict__ bytes, size_t count, size_t nb, int b1, int zcash,
    ProofAffine<typename Tower<PP>::Fq, typename Tower<PP>::F2>* __restrict__ proofs, uint8_t* __restrict__ pok) {
  using Fq = typename Tower<PP>::Fq;
  using F2 = typename Tower<PP>::F2;
  constexpr size_t S1 = PointCodec<Fq>::SIZE, SP = 4 * S1;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nb) {
    if (t >= count) return;
    Affine<F2> r;
    const bool good = decode_checked_point<PP, true>(bytes + t * SP + S1, b1, zcash, &r);
    proofs[t].B = r;
    pok[3 * t + 1] = (uint8_t)good;
  } else {
    const size_t u = t - nb, i = u >> 1;
    if (i >= count) return;
    const bool is_c = (u & 1) != 0;
    Affine<Fq> r;
    const bool good = decode_checked_point<PP, false>(bytes + i * SP + (is_c ? 3 * S1 : 0), b1, zcash, &r);
    if (is_c) proofs[i].C = r;
    else proofs[i].A = r;
    pok[3 * i + (is_c ? 2 : 0)] = (uint8_t)good;
  }
}

// Second launch, one lane per proof: canonical little-endian Fr bytes [count][n_inputs][32] -> Montgomery form (0 for a value
// that is not below r), and valid0[i] = the three point verdicts and every input of proof i in range
template <class FrP>
__global__ __launch_bounds__(64) void verify_stage_inputs_kernel(const uint8_t* __restrict__ in_bytes, size_t n_inputs, size_t count,
                                                                const uint8_t* __restrict__ pok, Fp<FrP>* __restrict__ inputs,
                                                                uint8_t* __restrict__ valid0) {
  using Fr = Fp<FrP>;
  static_assert(Fr::N == 8, "a public input is 32 bytes");
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  bool ok = pok[3 * i] && pok[3 * i + 1] && pok[3 * i + 2];
#pragma unroll 1
  for (size_t t = 0; t < n_inputs; t++) {
    const uint8_t* p = in_bytes + (i * n_inputs + t) * 32;
    Fr x;
#pragma unroll
    for (int j = 0; j < 8; j++)
      x.v[j] = (uint32_t)p[4 * j] | ((uint32_t)p[4 * j + 1] << 8) | ((uint32_t)p[4 * j + 2] << 16) | ((uint32_t)p[4 * j + 3] << 24);
    const bool in_range = x.is_canonical();
    ok = ok && in_range;
    inputs[i * n_inputs + t] = in_range ? x.to_mont() : Fr::zero();
  }
  valid0[i] = (uint8_t)ok;
}

// valid[i] &= valid0[i]: the staged verdicts join the ones the unchecked verifier's own kernels wrote
template <class PP>
__global__ __launch_bounds__(256) void verify_valid_and_kernel(uint8_t* __restrict__ valid, const uint8_t* __restrict__ valid0,
                                                              size_t count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) valid[i] = (uint8_t)(valid[i] && valid0[i]);
}

}  // namespace zk
