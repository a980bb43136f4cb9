// Host-side check of the lane-group index map of base_mul_few_kernel (csrc/base_mul_few_map.hpp): for every window count
// 1..FEW_MAX_WIN the lanes of a group take every window below nwin exactly once, few_digits extracts exactly the byte of
// that window from the canonical limbs (random scalars against plain byte indexing, for 8 limbs and fewer), and the
// reduction tree pairs every lane once per level so that lane 0 ends with the sum of all FEW_LANES partial sums.
// Prints one line per violation and "N violations" last.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "base_mul_few_map.hpp"

using namespace zk;

static int bad = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      bad++;                                  \
      std::printf("violation: " __VA_ARGS__); \
      std::printf("\n");                      \
    }                                         \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

template <int NL>
static size_t check_digits() {
  size_t n = 0;
  for (int rep = 0; rep < 200; rep++) {
    uint32_t limbs[NL];
    for (int i = 0; i < NL; i++) limbs[i] = rep == 0 ? 0xffffffffu : rnd();
    uint8_t bytes[4 * NL];
    std::memcpy(bytes, limbs, sizeof(bytes));                   // little-endian host: byte w of the scalar
    for (int g = 0; g < FEW_LANES; g++) {
      const uint32_t d = few_digits<NL>(limbs, g);
      for (int k = 0; k < FEW_PER_LANE; k++) {
        const int w = few_window(g, k);
        const uint32_t want = w < 4 * NL ? bytes[w] : 0u;
        CHECK(((d >> (8 * k)) & 0xffu) == want, "limbs %d lane %d digit %d: %u, want %u", NL, g, k, (d >> (8 * k)) & 0xffu, want);
        CHECK(few_limb(g, k) == w / 4 && few_shift(g) == 8 * (w % 4), "lane %d digit %d: limb / shift of window %d", g, k, w);
        n++;
      }
    }
  }
  return n;
}

int main() {
  static_assert(few_window(3, 2) == 19 && few_sends(4, 2) && few_receives(0, 2) && few_partner(0, 2) == 4, "constexpr");
  static_assert(few_blocks(37) == 5 && few_blocks(0) == 0 && few_blocks(FEW_MAX_LEN) == 512, "grid");
  // every window below nwin exactly once
  size_t windows = 0;
  for (int nwin = 1; nwin <= FEW_MAX_WIN; nwin++) {
    std::vector<int> seen(nwin, 0);
    for (int g = 0; g < FEW_LANES; g++)
      for (int k = 0; k < FEW_PER_LANE; k++) {
        const int w = few_window(g, k);
        CHECK(w >= 0 && w < FEW_MAX_WIN, "lane %d digit %d: window %d out of range", g, k, w);
        if (w < nwin) seen[w]++, windows++;
      }
    for (int w = 0; w < nwin; w++) CHECK(seen[w] == 1, "nwin %d: window %d taken %d times", nwin, w, seen[w]);
  }
  const size_t digits = check_digits<8>() + check_digits<7>() + check_digits<6>() + check_digits<4>();
  // the tree: masks of the lanes whose partial sums a lane holds
  uint32_t holds[FEW_LANES];
  for (int g = 0; g < FEW_LANES; g++) holds[g] = 1u << g;
  for (int v = 0; v < FEW_LEVELS; v++) {
    for (int g = 0; g < FEW_LANES; g++) {
      CHECK(!(few_sends(g, v) && few_receives(g, v)), "level %d lane %d sends and receives", v, g);
      if (!few_receives(g, v)) continue;
      const int p = few_partner(g, v);
      CHECK(p < FEW_LANES && few_sends(p, v), "level %d lane %d: partner %d does not send", v, g, p);
      if (p >= FEW_LANES) continue;
      CHECK((holds[g] & holds[p]) == 0, "level %d lane %d: partner %d holds a sum twice", v, g, p);
      holds[g] |= holds[p];
    }
    int senders = 0;
    for (int g = 0; g < FEW_LANES; g++) senders += few_sends(g, v);
    CHECK(senders == (FEW_LANES >> (v + 1)), "level %d: %d senders", v, senders);
  }
  CHECK(holds[0] == (1u << FEW_LANES) - 1, "lane 0 ends with the sums %x", holds[0]);
  // a group never straddles two workgroups and the grid covers len scalars with no workgroup to spare
  CHECK(FEW_BLOCK % FEW_LANES == 0, "block / lanes");
  for (size_t len = 1; len <= 2 * (size_t)FEW_BLOCK; len++) {
    const size_t nb = few_blocks(len), per = FEW_BLOCK / FEW_LANES;
    CHECK(nb * per >= len && (nb - 1) * per < len, "len %zu: %zu workgroups", len, nb);
  }
  std::printf("windows %zu digits %zu\n", windows, digits);
  std::printf("%d violations\n", bad);
  return bad != 0;
}
