// Host-side check of csrc/pairing_rlc_plan.hpp, the part of zk_groth16_verify_all that needs no device.  Built and run by
// tests/test_verify_all_plan.py with the host compiler.
//   rand <64 hex digits of seed> <index>...   prints "r <index> <w0> <w1> <w2> <w3>" (hex words) per index
//   zero                                      prints "zero ok" when a zero draw is replaced by 1 and nothing else is touched
//   plan <nmax>                               checks gt_fold_plan(n) for n = 1 .. nmax, prints "plan <n> <G> <len> <empty
//                                             groups>" for every n and "<k> violations" last
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pairing_rlc_plan.hpp"
using namespace zk;

static long bad = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (bad++ < 40) printf("FAIL %s  [n = %zu]\n", #cond, n);            \
    }                                                                      \
  } while (0)

static int do_rand(int argc, char** argv) {
  if (argc < 3 || strlen(argv[2]) != 64) return 2;
  uint8_t seed[32];
  for (int i = 0; i < 32; i++) {
    unsigned v = 0;
    if (sscanf(argv[2] + 2 * i, "%2x", &v) != 1) return 2;
    seed[i] = (uint8_t)v;
  }
  const RlcKey key = rlc_key(seed);
  for (int a = 3; a < argc; a++) {
    const uint64_t idx = strtoull(argv[a], nullptr, 0);
    uint32_t r[4];
    rlc_randomizer(key, idx, r);
    printf("r %llu %08x %08x %08x %08x\n", (unsigned long long)idx, r[0], r[1], r[2], r[3]);
  }
  return 0;
}

// No seed is known whose draw is zero, so the rule is checked on the step that applies it: rlc_randomizer is
// rlc_from_block of the block (compared below on 1000 indices), and rlc_from_block maps four zero words to 1 and leaves
// every other draw, also one with a single low or high bit, as it is.
static int do_zero() {
  uint8_t seed[32] = {0};
  const RlcKey key = rlc_key(seed);
  for (uint64_t i = 0; i < 1000; i++) {
    uint32_t r[4], want[4], blk[16];
    rlc_randomizer(key, i, r);
    chacha20_block(key.w, i, RLC_NONCE, blk);
    rlc_from_block(blk, want);
    if (memcmp(r, want, 16) != 0) return 1;
  }
  const uint32_t cases[4][16] = {{0, 0, 0, 0, 7, 7, 7, 7}, {1, 0, 0, 0}, {0, 0, 0, 0x80000000u}, {0, 2, 0, 0, 9}};
  const uint32_t want[4][4] = {{1, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 0x80000000u}, {0, 2, 0, 0}};
  for (int c = 0; c < 4; c++) {
    uint32_t r[4];
    rlc_from_block(cases[c], r);
    if (memcmp(r, want[c], 16) != 0) return 1;
  }
  printf("zero ok\n");
  return 0;
}

static size_t ceil_sqrt(size_t n) {
  size_t s = 0;
  while (s * s < n) s++;
  return s;
}

static int do_plan(size_t nmax) {
  for (size_t n = 1; n <= nmax; n++) {
    const GtFoldPlan p = gt_fold_plan(n);
    const size_t bound = ceil_sqrt(n) + 1;
    CHECK(p.n == n && p.G >= 1 && p.len >= 1);
    CHECK(p.G <= bound);
    CHECK(p.len <= bound);
    std::vector<int> seen(n, 0);
    size_t empties = 0, longest = 0;
    bool past = false;
    for (size_t g = 0; g < p.G; g++) {
      const size_t b = p.begin(g), e = p.end(g);
      CHECK(b <= e && e <= n);
      CHECK(p.empty(g) == (b == e));
      if (p.empty(g)) empties++, past = true;
      else CHECK(!past);                              // empty groups come last
      if (e - b > longest) longest = e - b;
      for (size_t t = b; t < e; t++) seen[t]++;
    }
    CHECK(longest <= p.len && longest <= bound);
    for (size_t t = 0; t < n; t++) CHECK(seen[t] == 1);
    // what the kernel computes from (n, G, len) alone is the same range
    for (size_t g = 0; g < p.G; g++) {
      const size_t lo = g * p.len < n ? g * p.len : n, hi = (g + 1) * p.len < n ? (g + 1) * p.len : n;
      CHECK(lo == p.begin(g) && hi == p.end(g));
    }
    printf("plan %zu %zu %zu %zu\n", n, p.G, p.len, empties);
  }
  const GtFoldPlan z = gt_fold_plan(0);
  if (z.G != 0 || z.len != 0) bad++;
  printf("%ld violations\n", bad);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "rand")) return do_rand(argc, argv);
  if (argc >= 2 && !strcmp(argv[1], "zero")) return do_zero();
  if (argc >= 3 && !strcmp(argv[1], "plan")) return do_plan((size_t)strtoull(argv[2], nullptr, 0));
  return 2;
}
