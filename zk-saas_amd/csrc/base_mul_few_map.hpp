// Lane-group index map of base_mul_few_kernel (base_mul_few.hpp): FEW_LANES lanes share one scalar.  Host-only code may
// include this header alone (tests/native/base_mul_few_map_host_test.cpp).
//
// Windows: the scalar has nwin 8-bit windows; lane g of a group takes the windows g, g + FEW_LANES, g + 2 FEW_LANES, ...
// below nwin -- window w = g + FEW_LANES k is byte (g & 3) of limb 2 k + (g >> 2) of the canonical scalar, so the K =
// FEW_MAX_WIN / FEW_LANES digits of a lane come from limbs with compile-time indices.
// Tree: FEW_LEVELS levels; at level v (stride s = 1 << v) the lanes with g % 2s == s send their partial sum and the lanes
// with g % 2s == 0 add the sum of lane g + s to their own; lane 0 holds the total after the last level.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ZK_FEW_HD __host__ __device__ inline
#else
#define ZK_FEW_HD inline
#endif

namespace zk {

constexpr int FEW_LANES = 8;          // lanes per scalar (a power of two that divides the wave)
constexpr int FEW_LEVELS = 3;         // log2(FEW_LANES)
constexpr int FEW_BLOCK = 64;         // one wave per workgroup: FEW_BLOCK / FEW_LANES scalars
constexpr int FEW_MAX_WIN = 32;       // 8-bit windows of a scalar of at most 8 limbs
constexpr int FEW_PER_LANE = FEW_MAX_WIN / FEW_LANES;
constexpr size_t FEW_MAX_LEN = 4096;  // zk_base_mul_few takes at most this many scalars (zk_base_mul above it)
static_assert((1 << FEW_LEVELS) == FEW_LANES && FEW_BLOCK % FEW_LANES == 0 && FEW_LANES == 8, "lane-group geometry");

// k-th window of lane g (may be >= nwin: the lane skips it)
ZK_FEW_HD constexpr int few_window(int g, int k) { return g + FEW_LANES * k; }
// limb and bit offset of that window in the canonical little-endian 32-bit limbs
ZK_FEW_HD constexpr int few_limb(int g, int k) { return 2 * k + (g >> 2); }
ZK_FEW_HD constexpr int few_shift(int g) { return 8 * (g & 3); }
// the digits of lane g, digit k in byte k: even limbs feed the lanes 0..3, odd limbs the lanes 4..7 (limb indices are
// compile-time constants: the kernel keeps the scalar in registers)
template <int NL>
ZK_FEW_HD uint32_t few_digits(const uint32_t* limbs, int g) {
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < FEW_PER_LANE; k++) {
    const uint32_t lo = 2 * k < NL ? limbs[2 * k < NL ? 2 * k : 0] : 0u;
    const uint32_t hi = 2 * k + 1 < NL ? limbs[2 * k + 1 < NL ? 2 * k + 1 : 0] : 0u;
    const uint32_t v = (g >> 2) ? hi : lo;
    d |= ((v >> few_shift(g)) & 0xffu) << (8 * k);
  }
  return d;
}
// tree roles at level v
ZK_FEW_HD constexpr bool few_sends(int g, int v) { return (g & ((2 << v) - 1)) == (1 << v); }
ZK_FEW_HD constexpr bool few_receives(int g, int v) { return (g & ((2 << v) - 1)) == 0; }
ZK_FEW_HD constexpr int few_partner(int g, int v) { return g + (1 << v); }
// workgroups of a launch over len scalars
ZK_FEW_HD constexpr size_t few_blocks(size_t len) { return (len * FEW_LANES + FEW_BLOCK - 1) / FEW_BLOCK; }

}  // namespace zk
