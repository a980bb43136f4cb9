// Host-side check of csrc/ntt.hpp's make_ntt_plan (it sits above the __HIPCC__ guard) for every (log_n, tile bits) the
// engine can pass: tb = 8 for k = 8..14 and tb = 11 for k = 15..38 (fft1_tiled; k = 38 is the last size that fits the four
// passes of NttPlan).  Per plan: npass <= 4; the passes are contiguous from stage 0 to k; the first takes at most tb stages,
// a later one at most tb - 2; 0 <= cbits <= min(tb - rbits, s0); cbits >= 2 on a later pass (the ">= 4 adjacent columns" of
// the header's comment).  Outside the domain (k > tb + 3 (tb - 2), k < 0, tb < 3) the plan must come back empty with the
// memory around it untouched.  Prints one line per plan ("plan k tb npass  s0 s1 cbits ...") and ends with "N violations".
// Built and run by tests/test_ntt_plan.py, which also compares every line with tests/ntt_sizes.py.
#include <cstdio>
#include "ntt.hpp"
using namespace zk;

static int bad = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      bad++;                                                               \
      printf("VIOLATION k=%d tb=%d pass=%d: %s\n", k, tb, i, #cond);        \
    }                                                                      \
  } while (0)

static void check(int k, int tb) {
  // canaries around the plan: make_ntt_plan fills pass[] by index
  struct {
    int before[4];
    NttPlan p;
    int after[4];
  } box;
  for (int j = 0; j < 4; j++) box.before[j] = box.after[j] = 0x5a5a5a5a;
  box.p = make_ntt_plan(k, tb);
  const NttPlan& p = box.p;
  int i = -1;
  for (int j = 0; j < 4; j++) CHECK(box.before[j] == 0x5a5a5a5a && box.after[j] == 0x5a5a5a5a);
  CHECK(p.log_n == k);
  CHECK(p.npass >= 1 && p.npass <= 4);
  printf("plan %d %d %d ", k, tb, p.npass);
  int s = 0;
  for (i = 0; i < p.npass && i < 4; i++) {
    const NttPass& ps = p.pass[i];
    const int rbits = ps.s1 - ps.s0;
    printf(" %d %d %d", ps.s0, ps.s1, ps.cbits);
    CHECK(ps.s0 == s);
    CHECK(rbits >= 1);
    CHECK(rbits <= (i == 0 ? tb : tb - 2));
    CHECK(ps.cbits >= 0);
    CHECK(ps.cbits <= tb - rbits);
    CHECK(ps.cbits <= ps.s0);
    if (i > 0) CHECK(ps.cbits >= 2);
    s = ps.s1;
  }
  printf("\n");
  i = -1;
  CHECK(s == k);
}

// outside the domain (more than four passes, a negative size, a tile too small for a later pass) the plan is empty and
// nothing around it is touched
static void check_refused(int k, int tb) {
  struct {
    int before[4];
    NttPlan p;
    int after[4];
  } box;
  for (int j = 0; j < 4; j++) box.before[j] = box.after[j] = 0x5a5a5a5a;
  box.p = make_ntt_plan(k, tb);
  int i = -1;
  for (int j = 0; j < 4; j++) CHECK(box.before[j] == 0x5a5a5a5a && box.after[j] == 0x5a5a5a5a);
  CHECK(box.p.npass == 0);
  printf("refused %d %d\n", k, tb);
}

int main() {
  int plans = 0;
  for (int k = NTT_TILE_BITS_SMALL; k <= NTT_SMALL_MAX_LOG_N; k++, plans++) {
    if (ntt_tile_bits(k) != NTT_TILE_BITS_SMALL) bad++, printf("VIOLATION k=%d: tile bits\n", k);
    check(k, NTT_TILE_BITS_SMALL);
  }
  for (int k = NTT_SMALL_MAX_LOG_N + 1; k <= NTT_TILE_BITS + 3 * (NTT_TILE_BITS - 2); k++, plans++) {
    if (ntt_tile_bits(k) != NTT_TILE_BITS) bad++, printf("VIOLATION k=%d: tile bits\n", k);
    check(k, NTT_TILE_BITS);
  }
  for (int k = NTT_TILE_BITS + 3 * (NTT_TILE_BITS - 2) + 1; k <= 64; k++) check_refused(k, NTT_TILE_BITS);
  for (int k = NTT_TILE_BITS_SMALL + 3 * (NTT_TILE_BITS_SMALL - 2) + 1; k <= 64; k++) check_refused(k, NTT_TILE_BITS_SMALL);
  check_refused(-1, NTT_TILE_BITS);
  check_refused(5, 2);
  printf("plans %d\n", plans);
  printf("%d violations\n", bad);
  return bad != 0;
}
