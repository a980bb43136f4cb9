// Host-side check of the bit-slice index map of reduce stage B (csrc/msm_plan.hpp msm_slice_index / msm_slice_count):
// for every row count HI = 2^hb and column count LO = 2^lo_bits the enumeration of slice j must be exactly the indices
// with bit j set, each once, in increasing order, and row HI must fall to slice hb alone.
// Prints one line per violation and "N violations" last.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "msm_plan.hpp"

using namespace zk;

static int bad = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      bad++;                              \
      std::printf("violation: " __VA_ARGS__); \
      std::printf("\n");                  \
    }                                     \
  } while (0)

// slice j over the indices [0, n): compare with the plain filter
static size_t check_slice(const char* what, int bits, uint32_t n, int j) {
  std::vector<uint32_t> want;
  for (uint32_t i = 0; i < n; i++)
    if ((i >> j) & 1u) want.push_back(i);
  const uint32_t cnt = msm_slice_count(n, j);
  CHECK(cnt == want.size(), "%s bits %d slice %d: count %u, want %zu", what, bits, j, cnt, want.size());
  std::vector<uint32_t> seen(n, 0);
  uint32_t prev = 0;
  for (uint32_t t = 0; t < cnt; t++) {
    const uint32_t i = msm_slice_index(t, j);
    CHECK(i < n, "%s bits %d slice %d: index %u of t = %u out of range", what, bits, j, i, t);
    if (i >= n) continue;
    CHECK((i >> j) & 1u, "%s bits %d slice %d: index %u lacks the bit", what, bits, j, i);
    CHECK(t == 0 || i > prev, "%s bits %d slice %d: index %u after %u", what, bits, j, i, prev);
    CHECK(t < want.size() && want[t] == i, "%s bits %d slice %d: t = %u gives %u", what, bits, j, t, i);
    seen[i]++;
    prev = i;
  }
  for (uint32_t i = 0; i < n; i++)
    CHECK(seen[i] == (((i >> j) & 1u) ? 1u : 0u), "%s bits %d slice %d: index %u seen %u times", what, bits, j, i, seen[i]);
  return cnt;
}

int main() {
  static_assert(msm_slice_index(0, 0) == 1 && msm_slice_index(5, 1) == 11 && msm_slice_count(129, 7) == 1, "constexpr");
  size_t slices = 0, indices = 0;
  for (int hb = 0; hb <= 10; hb++) {
    const uint32_t HI = 1u << hb;
    size_t with_top = 0;
    for (int j = 0; j <= hb; j++) {                   // rows 0..HI
      indices += check_slice("rows", hb, HI + 1, j);
      slices++;
      bool top = false;
      for (uint32_t t = 0; t < msm_slice_count(HI + 1, j); t++) top |= msm_slice_index(t, j) == HI;
      CHECK(top == (j == hb), "rows bits %d slice %d: row HI %s", hb, j, top ? "present" : "missing");
      with_top += top;
    }
    CHECK(with_top == 1, "rows bits %d: row HI in %zu slices", hb, with_top);
    CHECK(msm_slice_count(HI + 1, hb) == 1, "rows bits %d: top slice holds %u rows", hb, msm_slice_count(HI + 1, hb));
  }
  for (int lb = 0; lb <= 10; lb++) {
    const uint32_t LO = 1u << lb;
    for (int j = 0; j < lb; j++) {                    // columns 0..LO-1
      const size_t c = check_slice("columns", lb, LO, j);
      CHECK(c == LO / 2, "columns bits %d slice %d: %zu columns", lb, j, c);
      indices += c;
      slices++;
    }
  }
  std::printf("slices %zu indices %zu\n", slices, indices);
  std::printf("%d violations\n", bad);
  return bad != 0;
}
