// Host-compilable parts of zk_groth16_verify_all (pairing_rlc.hpp): how the randomizers of the batch check are derived from
// the call's seed, and how the product of the Miller values is split over lane groups.  No HIP here, so both are checked
// on the CPU (tests/native/rlc_host_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "prng.hpp"

namespace zk {

constexpr uint64_t RLC_NONCE = 0x5A4B524C43ull;

// the ChaCha20 key of a call: the 32 seed bytes as eight little-endian words
struct RlcKey {
  uint32_t w[8];
};
ZK_HD RlcKey rlc_key(const uint8_t* seed /* [32] */) {
  RlcKey k;
  for (int i = 0; i < 8; i++)
    k.w[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) |
             ((uint32_t)seed[4 * i + 3] << 24);
  return k;
}

// r_i = w0 | w1 << 32 | w2 << 64 | w3 << 96 of chacha20_block(key, counter = i, nonce = RLC_NONCE), as four little-endian
// words; a zero draw is replaced by 1 (a proof with randomizer 0 would not be checked at all)
ZK_HD void rlc_from_block(const uint32_t* blk, uint32_t r[4]) {
  for (int j = 0; j < 4; j++) r[j] = blk[j];
  if ((r[0] | r[1] | r[2] | r[3]) == 0) r[0] = 1;
}
ZK_HD void rlc_randomizer(const RlcKey& key, uint64_t i, uint32_t r[4]) {
  uint32_t blk[16];
  chacha20_block(key.w, i, RLC_NONCE, blk);
  rlc_from_block(blk, r);
}

// The product of n Miller values in two levels: G lane groups multiply `len` consecutive values each
// (pairing_gt_fold_kernel), the final exponentiation kernel multiplies the G results.  G = ceil(sqrt(n)) and
// len = ceil(n / G) <= G, so both chains are about sqrt(n) long where one group alone would run n products.  Group g takes
// [g len, min(n, (g + 1) len)); the last non-empty group may be partial, a group past the end is empty and yields 1.
struct GtFoldPlan {
  size_t n = 0, G = 0, len = 0;
  size_t begin(size_t g) const { return g * len < n ? g * len : n; }
  size_t end(size_t g) const { return (g + 1) * len < n ? (g + 1) * len : n; }
  bool empty(size_t g) const { return begin(g) >= n; }
};
inline GtFoldPlan gt_fold_plan(size_t n) {
  GtFoldPlan p;
  p.n = n;
  if (!n) return p;
  size_t G = 1;
  while (G * G < n) G++;
  p.G = G;
  p.len = (n + G - 1) / G;
  return p;
}

}  // namespace zk
