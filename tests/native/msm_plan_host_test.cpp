// Host-side check of csrc/msm_plan.hpp: the launch plan of the Pippenger MSM (windows, accumulate lanes, two-level sort,
// workspace layout, zeroed span, refusals) over a grid of the inputs the library can see.  Built and run by
// tests/test_msm_plan.py with the host compiler; the "win" lines it prints are compared there with tests/msm_digits.geometry.
// These are conditions a launch relies on, not measurements: a violation is a finding about the plan, to be reported.
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
#include "msm_plan.hpp"
using namespace zk;

static long bad = 0;
#define CHECK(cond)                                                                                         \
  do {                                                                                                      \
    if (!(cond)) {                                                                                          \
      if (bad++ < 40) printf("FAIL %s  [%s]\n", #cond, what);                                               \
    }                                                                                                       \
  } while (0)

// the five (scalar field, coordinate field) pairs the library instantiates; waves per SIMD as ACC_WAVES / SPLIT_WAVES
// (csrc/msm.hpp) give them: 4 on 8-limb base fields, 3 on 12-limb ones
struct Curve {
  const char* name;
  int bits, scalar_bytes, coord_bytes;
  bool g2;
  int waves;
};
static const Curve CURVES[] = {{"bn254 g1", 254, 32, 32, false, 4},
                               {"bn254 g2", 254, 32, 64, true, 4},
                               {"bls381 g1", 255, 32, 48, false, 3},
                               {"bls381 g2", 255, 32, 96, true, 3},
                               {"bls377 g1", 253, 32, 48, false, 3}};
constexpr size_t LDS_CU = 160 * 1024;      // the LDS of a gfx950 CU

static std::set<std::pair<int, int>> seen_windows;      // (scalar bits, requested width)

static void check_windows(const MsmWindows& w, int bits, const char* what) {
  CHECK(w.wide >= 1 && w.wide <= w.nwin);
  int sum = 0;
  for (int i = 0; i < w.nwin; i++) {
    CHECK(w.width(i) == w.c || w.width(i) == w.c - 1);
    CHECK(w.start(i) == sum);
    sum += w.width(i);
  }
  CHECK(sum == bits + 1);
  CHECK(w.start(w.nwin) == bits + 1);
}

static void check_plan(const MsmPlanIn& in, const MsmPlan& p, const char* what) {
  const int c_req = in.tab_c ? in.tab_c : msm_pick_c(in.scalar_bits, in.npts, in.c_force);
  if (in.c_force >= 2 && in.c_force <= 20 && !in.tab_c) CHECK(c_req == in.c_force);
  seen_windows.insert({in.scalar_bits, c_req});
  const MsmWindows w = MsmWindows::of(in.scalar_bits, c_req);
  CHECK(p.win.c == w.c && p.win.nwin == w.nwin && p.win.wide == w.wide);
  check_windows(p.win, in.scalar_bits, what);
  const int c = p.win.c, nwin = p.win.nwin;
  CHECK(p.sort_hi + p.sort_lo == c - 1);
  CHECK(p.B == 1u << (c - 1));
  CHECK(p.kwin == (in.tab_c ? 1 : nwin));
  CHECK(p.nsets == in.batch * p.kwin && p.nkeys == p.nsets * p.B);
  CHECK(p.max_sorted == in.npts * in.batch * nwin);
  CHECK(p.nsorts == ((in.vectors == 2 && !(in.tab_c && in.tab_no_identity)) ? 2u : 1u));
  if (p.big) {
    CHECK(p.sort_hi >= 1);
    CHECK(p.sort_lo >= 1 && p.sort_lo <= 12);
    CHECK(p.nbins_tot == p.nsets << p.sort_hi && p.nbins_tot <= (size_t)BIG_MAX_BINS);
    if (p.large) CHECK(p.ppt == 8 || p.ppt == 4 || p.ppt == 2 || p.ppt == 1);
    CHECK(p.hist_lds > 0 && p.hist_lds <= LDS_CU);
    CHECK(p.scatter_lds > 0 && p.scatter_lds <= LDS_CU);
    CHECK(p.binsort_lds > 0 && p.binsort_lds <= LDS_CU);
    CHECK(p.hist_ppt >= 1);
  }
  CHECK((uint64_t)p.nlanes * p.tmin >= p.max_sorted);
  CHECK(p.nlanes >= 1);

  // ---- workspace: 256-byte aligned regions in ascending order that do not overlap and end at the total
  const bool present[R_COUNT] = {true, true, p.big, true, true, true, true, true, true, p.big, p.big && p.wide_fmt, p.use_tcnt,
                                 true, true, true, true};
  size_t end = 0;      // end of the last region seen
  for (int id = 0; id < R_COUNT; id++) {
    const MsmRegion& r = p.r[id];
    CHECK((r.bytes > 0) == present[id]);
    if (id == R_SORT_END) {
      CHECK(end <= p.sort_region && p.sort_region - end < 256 && p.sort_region % 256 == 0);
      CHECK(p.ys == (p.nsorts == 2 ? p.sort_region : 0));
      CHECK(r.off == p.sort_region * p.nsorts);      // the per-vector regions start after every copy of the sort region
      end = r.off;
    }
    if (!r.bytes) continue;
    CHECK(r.off % 256 == 0);
    CHECK(r.off >= end);
    end = r.off + r.bytes;
  }
  CHECK(end <= p.ws_bytes && p.ws_bytes - end < 256 && p.ws_bytes % 256 == 0);
  CHECK(p.r[R_COUNTS].off == 0);
  CHECK(p.r[R_COUNTS].bytes >= p.nkeys * 4 && p.r[R_OFFSETS].bytes >= (p.nkeys + 1) * 4);
  CHECK(p.r[R_SORTED].bytes >= p.max_sorted * 4 && p.r[R_K0].bytes >= (size_t)p.nlanes * 4);
  CHECK(p.r[R_CANON].bytes >= in.npts * in.batch * in.scalar_bytes);

  // ---- the zeroed span: starts at a region, lies inside one sort copy, touches exactly heavy + bins / counts + heavy
  CHECK(p.zero_bytes % 4 == 0 && p.zero_off + p.zero_bytes <= p.sort_region);
  const MsmRegion &cn = p.r[R_COUNTS], &hv = p.r[R_HEAVY], &bn = p.r[R_BINS];
  if (p.big) {
    CHECK(p.zero_off == hv.off);
    CHECK(p.zero_off + p.zero_bytes == bn.off + (p.nbins_tot + 1) * 4);      // bin counters and the ticket word behind them
    CHECK(p.zero_off + p.zero_bytes <= bn.off + bn.bytes);
    CHECK(bn.bytes == msm_bins_words(p.nbins_tot) * 4);
    // nothing lies between the heavy list and the bins
    CHECK(bn.off - (hv.off + hv.bytes) < 256);
  } else {
    CHECK(p.zero_off == cn.off);
    CHECK(p.zero_off + p.zero_bytes == hv.off + 16);                          // the counts and the heavy-bucket counter
    CHECK(p.zero_off + p.zero_bytes <= hv.off + hv.bytes);
    CHECK(hv.off - (cn.off + cn.bytes) < 256);
  }
  CHECK(hv.bytes == msm_heavy_cap(p.nlanes) * 8 + 16);

  // ---- pinned buffer and the fold's part
  CHECK(p.out_bytes == (size_t)p.vectors * p.nsets * c * 4 * in.coord_bytes);
  CHECK(p.pinned_bytes >= p.out_bytes + 8 * p.nsorts);
  const MsmFoldGeo& f = p.fold;
  CHECK(f.win.c == c && f.win.nwin == nwin && f.win.wide == p.win.wide && f.kwin == p.kwin && f.lo_bits == p.lo_bits);
  CHECK(f.batch == (int)in.batch && f.nb == (int)p.vectors && f.nsorts == (int)p.nsorts && f.tabbed == (in.tab_c != 0));
  CHECK(f.stats_off == p.out_bytes && f.offered == in.npts * in.batch * p.vectors * nwin && f.g2 == in.g2);
  CHECK(p.lo_bits == c / 2 && p.nslices == c);
}

int main() {
  const size_t NPTS[] = {1, 50, 1000, (1u << 14) - 1, 1u << 14, 119000, 1u << 17, 1u << 20, (1u << 22) - 1, 1u << 22,
                         1u << 23, 1u << 24, 1u << 26};
  const size_t BATCH[] = {1, 2, 4, 8, 16};
  const size_t BIGMIN[] = {0, (size_t)1 << 14, (size_t)1 << 40};
  long plans = 0, refused = 0, two_level = 0;
  char what[200];
  for (const Curve& cv : CURVES)
    for (size_t npts : NPTS)
      for (size_t batch : BATCH)
        for (int vectors = 1; vectors <= 2; vectors++)
          for (size_t bigmin : BIGMIN)
            // table-free at msm_c 0 and 2..20 (k = 0, 2..20); then tables of width 8..22 (k = 21..35), with and without identities
            for (int k = 0; k <= 35; k++) {
              if (k == 1) continue;
              for (int noid = 0; noid <= (k > 20 ? 1 : 0); noid++) {
                MsmPlanIn in;
                in.scalar_bits = cv.bits, in.scalar_bytes = cv.scalar_bytes, in.coord_bytes = cv.coord_bytes;
                in.g2 = cv.g2, in.acc_waves = cv.waves;
                in.npts = npts, in.batch = batch, in.vectors = vectors, in.bigsort_min = bigmin;
                if (k <= 20) in.c_force = k;
                else in.tab_c = MsmWindows::of(cv.bits, k - 13).c, in.tab_len = npts, in.tab_no_identity = noid != 0;
                snprintf(what, sizeof what, "%s npts=%zu batch=%zu vectors=%d bigsort_min=%zu msm_c=%d table=%d noid=%d", cv.name,
                         npts, batch, vectors, bigmin, in.c_force, k > 20 ? k - 13 : 0, noid);
                const MsmPlan p = msm_plan(in);
                const int nwin = p.win.nwin;
                // the refusals, stated independently
                const char* want = npts * batch >= ((size_t)1 << 31) ? "msm too large"
                                   : npts * batch * nwin >= ((size_t)1 << 32) ? "msm too large (points x windows >= 2^32)"
                                                                              : nullptr;
                CHECK((p.err == nullptr) == (want == nullptr));
                if (p.err && want) CHECK(!strcmp(p.err, want));
                {
                  // zk_msm_plan's four numbers are the plan's (a table-free launch of one vector)
                  int out[4];
                  msm_plan_of(in, out);
                  if (!in.tab_c && batch == 1 && vectors == 1)
                    CHECK(out[0] == p.win.c && out[1] == p.win.nwin && out[2] == (int)p.tmin && out[3] == (cv.g2 ? 28 : 10));
                }
                if (p.err) {
                  refused++;
                  continue;
                }
                plans++;
                two_level += p.big;
                check_plan(in, p, what);
              }
            }
  {
    // refusals outside the grid
    const char* what = "refusals";
    MsmPlanIn in;
    in.scalar_bits = 254, in.scalar_bytes = 32, in.coord_bytes = 32, in.acc_waves = 4, in.bigsort_min = 1 << 14;
    in.npts = 1000;
    in.batch = 0;
    CHECK(msm_plan(in).err && !strcmp(msm_plan(in).err, "bad msm batch"));
    in.batch = 17;
    CHECK(msm_plan(in).err && !strcmp(msm_plan(in).err, "bad msm batch"));
    in.batch = 16;
    CHECK(!msm_plan(in).err);
    in.npts = (size_t)1 << 27;      // x 16 = 2^31
    CHECK(msm_plan(in).err && !strcmp(msm_plan(in).err, "msm too large"));
    in.batch = 1, in.npts = ((size_t)1 << 31) - 1, in.c_force = 20;      // 13 windows
    CHECK(msm_plan(in).err && !strcmp(msm_plan(in).err, "msm too large (points x windows >= 2^32)"));
    in.npts = (size_t)1 << 31;
    CHECK(msm_plan(in).err && !strcmp(msm_plan(in).err, "msm too large"));
    in.npts = 0, in.batch = 3;      // nothing to launch: no refusal, the fold still learns the batch
    CHECK(!msm_plan(in).err && msm_plan(in).fold.batch == 3);
  }
  // every window layout a plan used, and every requested width a table or an option can ask for
  for (const Curve& cv : CURVES)
    for (int c_req = 2; c_req <= 22; c_req++) seen_windows.insert({cv.bits, c_req});
  for (const auto& bw : seen_windows) {
    const MsmWindows w = MsmWindows::of(bw.first, bw.second);
    const char* what = "windows";
    check_windows(w, bw.first, what);
    printf("win %d %d %d %d %d :", bw.first, bw.second, w.c, w.nwin, w.wide);
    for (int i = 0; i < w.nwin; i++) printf(" %d", w.width(i));
    printf(" :");
    for (int i = 0; i < w.nwin; i++) printf(" %d", w.start(i));
    printf("\n");
  }
  printf("plans %ld refused %ld two-level %ld\n", plans, refused, two_level);
  printf("%ld violations\n", bad);
  return bad != 0;
}
