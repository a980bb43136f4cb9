// Fixed-base multiplication for a FEW scalars (the MSM masks of a batch of proofs: 64 B G1 and 16 B G2 scalars at n = 8):
// fixed_base_mul_kernel (groth16.hpp) gives a lane a whole scalar -- 32 dependent mixed additions, right at 2^17 scalars
// and a serial chain on a handful of waves here.  This kernel gives a scalar to FEW_LANES = 8 lanes: each lane adds the
// table entries of its 4 windows (table[w][d-1] = d 256^w Base, the 8-bit table of Engine::base_mul_t), then the group
// folds its 8 partial sums in 3 levels over LDS -- 4 mixed + 3 full additions deep instead of 32.  The tree uses the
// complete adder (xyzz_add: equal, opposite and identity operands), since partial sums are arbitrary points.  Output is
// Jacobian: no inversion.  Index map: base_mul_few_map.hpp.  Instantiated per (curve, group) in the msm_<curve>_g<k>.hip
// translation units (base_mul_few_launch, msm_impl.hpp), so the Fq2 form is compiled with the G2 units' inline products.
#pragma once
#include "base_mul_few_map.hpp"
#include "ec.hpp"
#include "ntt.hpp"

namespace zk {
#if defined(__HIPCC__)

template <class FrP, class Fld>
__global__ __launch_bounds__(FEW_BLOCK) void base_mul_few_kernel(const Fp<FrP>* __restrict__ scalars, size_t len,
                                                                const Affine<Fld>* __restrict__ table, int nwin,
                                                                Jacobian<Fld>* __restrict__ out) {
  static_assert(FrP::N <= 8, "scalar fields have at most 8 limbs");
  __shared__ XYZZ<Fld> sh[FEW_BLOCK];
  const size_t i = ((size_t)blockIdx.x * FEW_BLOCK + threadIdx.x) / FEW_LANES;
  const int g = (int)(threadIdx.x % FEW_LANES);
  const bool live = i < len;                                // group-uniform; dead groups still meet the barriers
  XYZZ<Fld> acc = XYZZ<Fld>::identity();
  if (live) {
    const Fp<FrP> s = load_elem(scalars + i).from_mont();
    uint32_t digs = few_digits<FrP::N>(s.v, g);
#pragma unroll 1
    for (int k = 0; k < FEW_PER_LANE; k++, digs >>= 8) {
      const uint32_t d = digs & 0xffu;
      const int w = few_window(g, k);
      if (d && w < nwin) {
        const Affine<Fld> t = load_elem(table + (size_t)w * 255 + (d - 1));
        acc = xyzz_madd(acc, t.x, t.y);
      }
    }
  }
#pragma unroll 1
  for (int v = 0; v < FEW_LEVELS; v++) {
    if (few_sends(g, v)) sh[threadIdx.x] = acc;
    __syncthreads();
    if (live && few_receives(g, v)) acc = xyzz_add(acc, sh[threadIdx.x + (1 << v)]);
    __syncthreads();
  }
  if (live && g == 0) store_elem(out + i, xyzz_to_jacobian(acc));
}

#endif  // __HIPCC__
}  // namespace zk
