// The launch plan of a Pippenger MSM as a value: window geometry, accumulate lanes, the plan of the two-level sort and
// the workspace layout, computed by ONE pure function from plain inputs (no clocks, no globals, no registry lookups).
// msm_launch (msm_impl.hpp), zk_msm_plan (msm_plan_of), zk_msm_precompute (MsmWindows) and the host fold all read it.
// Host-only integer arithmetic: no HIP header, compiles with the host compiler alone (tests/native/msm_plan_host_test.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace zk {

constexpr size_t MSM_RANGE_MIN = 20, MSM_RANGE = 64;        // entries per accumulate lane: fewest (small MSMs), most
                                                            // (SHA-256 proof, same box, round 5: 14 -> 622-626, 26 -> 629-630
                                                            // against 646-649 proofs/s at 20)
constexpr size_t MSM_RANGE_MIN_G2 = 16, MSM_RANGE_G2 = 64;  // ... per lane quad of the extension-field kernel (32 until
                                                            // round 4; C5: 1.303 s at 32, 1.286 at 64, 1.280 at 128)
constexpr uint32_t FIN_SEQ = 16;      // a bucket spread over more accumulate lanes than this is summed by a workgroup
constexpr int MSM_MAXB = 16;          // most scalar vectors of one launch (msm.hpp MsmScalars)

// two-level sort (msm.hpp "big sort")
constexpr int BIG_HI = 8;                 // top bucket bits of a bin when nothing else decides (msm_big_hi)
constexpr int BIG_MAX_BINS = 8192;
constexpr int BIG_THREADS = 256;          // histogram tiles; scatter / binsort: 256 (small launches) or 1024
constexpr int BIG_PTS_PER_THREAD = 8;     // most points per thread (scalars are held in registers by the scatter)
constexpr int BIG_EPT = 16;               // entries per thread and chunk of the bin sort
constexpr size_t BIG_LDS_MAX = 156 * 1024;
inline int msm_big_hi(size_t nsets) {
  int hi = BIG_HI;
  while (hi > 0 && (nsets << hi) > (size_t)BIG_MAX_BINS) hi--;
  return hi;
}
// Layout of the bins block (uint32): counts[nbins], ticket, base[nbins + 1], cursor[nbins]
constexpr size_t msm_bins_words(size_t nbins) { return 3 * nbins + 2; }

// three-launch scan of the atomics sort (msm.hpp "scan")
constexpr int ISCAN_THREADS = 256;
constexpr int ISCAN_PER = 8;
constexpr int ISCAN_BLOCK = ISCAN_THREADS * ISCAN_PER;

// Bit slices of reduce stage B (msm.hpp msm_reduce_b_kernel): slice j sums the rows (or columns) whose index has bit j
// set.  The quads of a slice enumerate exactly those indices -- the t-th of them is t with a 1 inserted at bit position
// j -- instead of walking every index and skipping half.  Host and device: the kernel and tests/native read the same map.
#if defined(__HIPCC__)
#define ZK_PLAN_HD __host__ __device__
#else
#define ZK_PLAN_HD
#endif
ZK_PLAN_HD constexpr uint32_t msm_slice_index(uint32_t t, int j) {
  return ((t >> j) << (j + 1)) | (1u << j) | (t & ((1u << j) - 1u));
}
// how many indices in [0, n) have bit j set (rows: n = HI + 1, so that the single index HI = 2^hb falls to slice hb alone;
// columns: n = LO)
ZK_PLAN_HD constexpr uint32_t msm_slice_count(uint32_t n, int j) {
  const uint32_t rem = n & ((2u << j) - 1u);
  return ((n >> (j + 1)) << j) + (rem > (1u << j) ? rem - (1u << j) : 0u);
}

// capacity of the heavy list (entries) and of hpart[] (virtual workgroups) for a launch of nlanes accumulate lanes
// (msm.hpp "HEAVY LIST")
inline size_t msm_heavy_cap(size_t nlanes) { return nlanes / FIN_SEQ + 8; }
inline size_t msm_heavy_vcap(size_t nlanes) { return nlanes / FIN_SEQ + nlanes / 256 + 8; }

// BITS+1 bits (room for the signed-digit carry) are spread EVENLY over the windows: `wide` windows of c bits and
// nwin-wide of c-1.  A plain c-bit split leaves a top window of a few bits (254 = 19*13 + 7) whose 64 buckets
// each receive npts/64 points: hot atomics in the sort, long chains, and a heavy-bucket pass in every MSM.
struct MsmWindows {
  int c = 0, nwin = 0, wide = 0;                  // widest window; windows; windows [0, wide) have c bits, 1 <= wide <= nwin
  static MsmWindows of(int scalar_bits, int c_req) {
    const int T = scalar_bits + 1;
    MsmWindows w;
    w.nwin = (T + c_req - 1) / c_req;
    w.c = (T + w.nwin - 1) / w.nwin;
    w.wide = T - w.nwin * (w.c - 1);
    return w;
  }
  int width(int w) const { return w < wide ? c : c - 1; }
  int start(int w) const { return w * (c - 1) + std::min(w, wide); }      // bit position of window w
};

// Window width: minimise nwin * (npts + 4 * buckets) -- mixed additions plus the per-bucket reduction work --
// with nwin = ceil((BITS+1)/c) windows of evenly spread width (MsmWindows); ties go to the wider window
// (more buckets = more lanes with shorter chains).
inline int msm_pick_c(int scalar_bits, size_t npts, int c_force = 0) {
  if (c_force >= 2 && c_force <= 20) return c_force;      // zk_ctx_set_option "msm_c" / "msm_c_g2" (tests force widths)
  int best = 4;
  double best_cost = 1e300;
  for (int c = 4; c <= 20; c++) {                     // > 17 only pays from ~2^25 points on (cost model below)
    int nwin = (scalar_bits + c) / c;
    int ceff = (scalar_bits + nwin) / nwin;        // widest window after spreading BITS+1 bits over nwin windows
    // per-bucket work is priced at 4 additions up to 17 bits (tuned on 10^5..10^7 points) and at 10 above: measured
    // on BLS12-381, 20-bit windows lose 13% at 2^24 points and win 8% at 2^26
    double cost = (double)nwin * ((double)npts + (ceff > 17 ? 10.0 : 4.0) * (double)((size_t)1 << (ceff - 1)));
    if (cost <= best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}

// Accumulate lanes of a launch with at most `max_entries` sorted entries (msm.hpp "balanced partition"): entries per
// lane `t` and the lane count that covers max_entries at that length.  Measured on batches of 1 / 2 / 4 / 8 119k-point
// MSMs alone on the chip (1.9 M .. 15 M entries; the chip holds 196 608 lanes at three waves per SIMD, 262 144 at the four
// the BN254 kernel is compiled for since round 4;
// profiles/r03_range_sweep.txt): what matters is how many ROUNDS of waves a launch makes -- >= 1.6 rounds run at
// 98-116 G multiplications/s, exactly one round at 79 (a grid that just fills the chip leaves the dispatcher no slack and
// all its waves march in step), fewer than one underfills -- while every lane boundary costs one full addition (14
// multiplications; 42 in G2) in the finalize kernel.  So: ~2.4 rounds, but never fewer than `lo` entries per lane (small
// launches: the MSMs of ONE proof run four at a time and fill the chip together) nor more than `hi`.
struct MsmLanes {
  uint32_t nlanes, tmin, cap;
};
inline MsmLanes msm_pick_lanes(size_t max_entries, int waves, bool pair, int lanes_per_range = 0) {
  if (!lanes_per_range) lanes_per_range = pair ? 2 : 1;
  const size_t cap = (size_t)1024 * waves * (64 / lanes_per_range);
  const size_t lo = pair ? MSM_RANGE_MIN_G2 : MSM_RANGE_MIN;
  const size_t hi = pair ? MSM_RANGE_G2 : MSM_RANGE;
  size_t t = std::min(hi, std::max(lo, (size_t)((double)max_entries / (2.4 * (double)cap))));
  size_t nl = std::max<size_t>(1, (max_entries + t - 1) / t);
  // between one and two rounds at this length msm_range_len splits the entries over TWO rounds of shorter ranges: the
  // launch needs the lanes of two rounds then (found by the 2^18-point BLS12-381 prover test: 4.4 M entries at 20 per
  // lane made 222 823 lanes, the two-round length of 12 covered 2.7 M entries and the rest was never added)
  if (max_entries >= cap * t && max_entries < 2 * cap * t && (max_entries + 2 * cap - 1) / (2 * cap) >= 12)
    nl = std::max(nl, 2 * cap);
  return MsmLanes{(uint32_t)nl, (uint32_t)t, (uint32_t)cap};
}

// Window bits of a new fixed-base table (zk_msm_precompute) by the vector's length, unless zk_ctx_set_option
// "msm_table_c" / "msm_table_c_g2" asks for a width.  A table folds all windows into ONE set of 2^(c-1) buckets, so a
// bucket receives len * nwin / 2^(c-1) entries: once that is more than FIN_SEQ (16) accumulate ranges long, every
// bucket goes through the heavy-bucket path meant for degenerate scalars and the MSM is 2-3x slower than table-free
// (measured, tools/tab_c3.py, G1 d_msm over 2^19 / 2^20 / 2^23 points: c = 16 2.53 / 3.48 / 18.8 ms, c = 17 1.10 /
// 1.95 / 20.7, c = 20 1.45 / 2.2 / 11.8; table-free 1.59 / 2.77 / 12.7; below 2^19 points c = 16 is best: 0.78 against
// 1.15 ms table-free at 2^18).  G1: 15 bits (17 windows, 16 384 buckets) up to 2^17 points -- the SHA-256 proof's four G1
// MSMs: 6 % more mixed additions than 16 bits but half the buckets in the reduction every chain ends with: 634 / 649 /
// 653 / 651 vs 630 / 639 / 638 / 638 proofs/s, same box, round 5; 14 bits already sends every bucket down the heavy path:
// 512-542 --, 16 bits below 2^19 points, 18 below 2^22 (re-rounded to evenly spread windows: 17 bits
// = 15 windows on BN254's 254-bit Fr, 18 bits on BLS12-381's 255-bit Fr), 20 (13 windows) from there.
// G2: 15 bits = 17 windows, 16 384 buckets below 2^20 points (6 % more mixed additions than 16 bits but half the
// buckets in the G2 reduction, the latency chain a proof ends with: 458-477 vs 423-453 proofs/s, same box), 19 (14
// windows) from there (2^21 points: 11.1 ms against 17.8 at 15 bits and 11.8 table-free).
inline int table_c_auto(size_t len, bool g2) {
  if (g2) return len < ((size_t)1 << 20) ? 15 : 19;
  return len <= ((size_t)1 << 17) ? 15 : len < ((size_t)1 << 19) ? 16 : len < ((size_t)1 << 22) ? 18 : 20;
}

// What the host fold needs of a launch (MsmPending::fold, msm_fold_batch)
struct MsmFoldGeo {
  MsmWindows win;
  int kwin = 0;                  // bucket sets per scalar vector: with a table all windows share one
  int lo_bits = 0;               // reduce stage A / B: column slices of a bucket set (the other c - lo_bits are row slices)
  bool tabbed = false;           // fixed-base table: one bucket set
  int batch = 1;                 // scalar vectors of the launch (results: [base vector][batch])
  int nb = 1;                    // base vectors
  int nsorts = 1;                // sorts (2: one per base vector, their identities differ)
  size_t stats_off = 0;          // statistics: where the sorts' entry counts land in the pinned buffer, behind the slices
  size_t offered = 0;            // (point, window) pairs offered to the sort
  bool g2 = false;
};

// The bucket geometry of a launch: two launches whose geometries are equal fill bucket arrays that can be added bucket by
// bucket (msm.hpp "SHARED BUCKET SET"): bucket k of either holds the points whose digit in the same window (of the same
// bit position and width) has the same magnitude.
struct MsmGeo {
  bool g2 = false;
  int c = 0, nwin = 0, kwin = 0, lo_bits = 0;
  size_t nsets = 0, nkeys = 0;
  uint32_t B = 0;
  bool operator==(const MsmGeo& o) const {
    return g2 == o.g2 && c == o.c && nwin == o.nwin && kwin == o.kwin && lo_bits == o.lo_bits && nsets == o.nsets &&
           nkeys == o.nkeys && B == o.B;
  }
  bool operator!=(const MsmGeo& o) const { return !(*this == o); }
};

struct MsmPlanIn {
  int scalar_bits = 0, scalar_bytes = 0;     // scalar field: bits of the modulus, bytes of an element
  int coord_bytes = 0;                       // bytes of one coordinate (an Fq2 element for G2)
  bool g2 = false;
  int acc_waves = 0;                         // waves per SIMD the accumulate kernel is compiled for (ACC_WAVES / SPLIT_WAVES)
  size_t npts = 0, batch = 1;
  int vectors = 1;                           // base vectors multiplied by the same scalars: 1 or 2
  int tab_c = 0;                             // fixed-base table registered for the base vector(s): its c, or 0 = none
  size_t tab_len = 0, tab_off = 0;           // ... points per table row, position of the launch's first point in a row
  bool tab_no_identity = false;              // ... no registered vector of the launch holds an identity
  int c_force = 0;                           // zk_ctx_set_option "msm_c" / "msm_c_g2" (0: the cost model)
  size_t bigsort_min = 0;                    // two-level sort from this many points on ("msm_bigsort_min")
  bool own_sorts = false;                    // two base vectors: a sort each even without identities (their scalars are scaled
                                             // differently: msm.hpp MsmShare::scale1)
};

// workspace regions, in layout order
enum MsmRegionId {
  // sort region (replicated per sort)
  R_COUNTS, R_HEAVY, R_BINS, R_CURSOR, R_OFFSETS, R_BT, R_SORTED, R_K0, R_CANON, R_TMP, R_TMP_LO, R_TCNT,
  // per base vector
  R_EDGE, R_BUCKETS, R_HPART, R_RC,
  R_COUNT,
  R_SORT_END = R_EDGE
};
struct MsmRegion {
  size_t off = 0, bytes = 0;     // bytes = 0: the launch has no such array
};

struct MsmPlan {
  const char* err = nullptr;     // refusal ("bad msm batch", "msm too large ..."): nothing below the lanes is filled
  size_t npts = 0, batch = 1;
  unsigned vectors = 1;
  MsmWindows win;
  uint32_t B = 0;                // buckets per set
  bool tabbed = false;
  int kwin = 0;                  // bucket sets per scalar vector: with a table all windows share one
  size_t nsets = 0, nkeys = 0;   // bucket sets, buckets of the launch
  size_t max_sorted = 0;         // most sorted entries (= mixed additions per base vector)
  uint32_t pre_stride = 0, pre_off = 0;      // table rows (0: no table), the launch's offset in a row
  // accumulate lanes (msm.hpp "balanced partition"): every lane adds the same number of sorted entries
  uint32_t nlanes = 0, tmin = 0, cap = 0;
  uint32_t vcap = 0;             // hpart[] entries per base vector
  // reduction geometry (msm.hpp "reduce stage A / B"): digit magnitudes k = hi * LO + lo in [1, B]
  int lo_bits = 0;               // LO = 2^lo_bits columns, HI = B / LO rows (+ the row of k = B)
  uint32_t red_groups = 0;
  int nslices = 0;               // (log2 HI + 1) row slices + lo_bits column slices
  size_t iscan_blocks = 0;
  bool no_identity = false;      // no base of the launch is the identity: the sort needs no identity test
  unsigned nsorts = 1;
  // ---- the two-level sort (msm.hpp "big sort"): workgroup shape, points per tile, bin split, entry format
  bool big = false;              // two-level sort (else: the atomics sort)
  bool large = false;            // multi-million-point launches: 1024-thread workgroups, one per CU
  int sthr = 0, ppt = 0;         // threads per scatter / binsort workgroup, points per scatter thread
  int sort_hi = 0, sort_lo = 0;  // bucket bits of a bin (level 1) / inside a bin (level 2): sort_hi + sort_lo = c - 1
  int idx_bits = 0;
  bool wide_fmt = false;         // entries of the first level: a word + a 16-bit low part (else one word)
  size_t nbl = 0;                // bins of one scalar vector
  size_t nbins_tot = 0;
  size_t stage_cap = 0, tile_pts = 0, tiles_big = 0;
  int wgroup = 0;                // windows per round of the staged scatter
  bool use_tcnt = false;         // the histogram pass hands its per-tile counts to the staged scatter
  int hist_ppt = 0;              // points per thread of the histogram's 256-thread tiles
  size_t hist_lds = 0, scatter_lds = 0, binsort_lds = 0;      // dynamic LDS of the three launches
  // ---- workspace
  MsmRegion r[R_COUNT];
  size_t sort_region = 0;        // bytes of one copy of the sort region
  size_t ys = 0;                 // byte distance between the two copies (0: one sort)
  size_t ws_bytes = 0;           // the slot's device scratch
  size_t zero_off = 0, zero_bytes = 0;       // what the zeroing launch clears (in every copy of the sort region)
  size_t out_bytes = 0;          // bit slices of all bucket sets (pinned)
  size_t pinned_bytes = 0;       // + the sorted-entry counts of the launch's sorts (msm statistics)
  MsmFoldGeo fold;
  MsmGeo geo() const { return MsmGeo{fold.g2, win.c, win.nwin, kwin, lo_bits, nsets, nkeys, B}; }
};

inline MsmPlan msm_plan(const MsmPlanIn& in) {
  MsmPlan p;
  const size_t npts = in.npts, batch = in.batch;
  const unsigned NB = in.vectors == 2 ? 2u : 1u;
  const bool tab = in.tab_c != 0;
  p.npts = npts, p.batch = batch, p.vectors = NB, p.tabbed = tab;
  if (batch < 1 || batch > (size_t)MSM_MAXB) {
    p.err = "bad msm batch";
    return p;
  }
  p.fold.batch = (int)batch;
  const MsmWindows win = MsmWindows::of(in.scalar_bits, tab ? in.tab_c : msm_pick_c(in.scalar_bits, npts ? npts : 1, in.c_force));
  const int c = win.c, nwin = win.nwin;
  p.win = win;
  p.B = 1u << (c - 1);
  const uint32_t B = p.B;
  const int kwin = p.kwin = tab ? 1 : nwin;
  const size_t nsets = p.nsets = batch * (size_t)kwin;
  const size_t nkeys = p.nkeys = nsets * B;
  const size_t max_sorted = p.max_sorted = npts * batch * nwin;
  // Extension field: a QUAD of lanes per range, one base-field value per lane (quad.hpp split_madd).  Rounds 2-3 held whole
  // Fq2 values per lane -- a pair of lanes per range, or one lane on large launches of 8-limb curves: 256 registers with
  // 13-99 spilled dwords, BLS12-381 G2 at a third of the multiplier's peak; those kernels are gone (measured with the quad
  // form: a 2^24-constraint BLS12-381 proof 1.42 -> 1.28 s, the SHA-256 proof 561 -> 593 proofs/s, table-free 395 -> 428)
  const MsmLanes ml = msm_pick_lanes(max_sorted, in.acc_waves, in.g2, in.g2 ? 4 : 0);
  const uint32_t nlanes = p.nlanes = ml.nlanes;
  p.tmin = ml.tmin, p.cap = ml.cap;
  if (npts * batch >= ((size_t)1 << 31)) p.err = "msm too large";
  else if (max_sorted >= ((size_t)1 << 32)) p.err = "msm too large (points x windows >= 2^32)";
  if (p.err || !npts) return p;
  p.pre_stride = tab ? (uint32_t)in.tab_len : 0u, p.pre_off = tab ? (uint32_t)in.tab_off : 0u;
  p.vcap = (uint32_t)msm_heavy_vcap(nlanes);
  const int lo_bits = p.lo_bits = c / 2;
  p.red_groups = (B >> lo_bits) + 1 + (1u << lo_bits);
  p.nslices = c;
  p.iscan_blocks = (nkeys + ISCAN_BLOCK - 1) / ISCAN_BLOCK;
  // identity bases are left out of the sort (msm.hpp MsmBaseId: the first sort-stage kernel gives them a zero scalar).
  // Two base vectors over the same scalars then get their OWN sorts (their identities differ: a fused sort could only
  // skip a point that is the identity in both) -- same kernels, grid.y = 2, the sort-stage arrays in two copies of one
  // workspace region (ZK_YSHIFT in the kernels).
  // registered vectors know whether they hold an identity at all (zk_msm_precompute): without one there is no mask
  p.no_identity = tab && in.tab_no_identity;
  const unsigned NS = p.nsorts = (NB == 2 && (!p.no_identity || in.own_sorts)) ? 2u : 1u;

  constexpr size_t large_min = (size_t)4 << 20;
  const bool large = p.large = npts * batch >= large_min;
  const int sthr = p.sthr = large ? 1024 : 256;
  // small launches: ~1024 tiles so that they still fill the chip, up to 16 points per thread
  int ppt = large ? BIG_PTS_PER_THREAD : 16;
  if (!large)
    while (ppt > 1 && ((npts + (size_t)sthr * ppt - 1) / ((size_t)sthr * ppt)) * batch < 1024) ppt >>= 1;
  const size_t stage_max = 16384;
  if (large && tab)
    while (ppt > 1 && (size_t)nwin * sthr * ppt > stage_max) ppt >>= 1;       // with a table the whole tile is one round
  p.ppt = ppt;
  // small launches: at least 7 low bits per bin (a table-free proof has 12-bit buckets in 20 sets: 8 top bits made 5120
  // bins of 16 buckets, one workgroup each -- measured 428 -> 442-447 proofs/s table-free with 5 top bits; the proof's
  // table sorts with 6 or 8 low bits instead of 7: no gain, profiles/r06_sort_bins_ab.txt)
  int sort_hi = std::min(msm_big_hi(nsets), std::max(1, c - 1 - 7));
  if (large) {
    // runs of level 1 are (tile entries per bucket set) / 2^hi long, runs of level 2 (chunk) / 2^lo: balance them
    auto lg = [](size_t v) { int l = 0; while (((size_t)1 << (l + 1)) <= v) l++; return l; };
    const int tp_eff = lg((size_t)sthr * ppt * (tab ? nwin : 1)), ch = lg((size_t)sthr * BIG_EPT);
    sort_hi = (c - 1 + tp_eff - ch + 1) / 2;
    if (sort_hi > c - 2) sort_hi = c - 2;
    if (c - 1 - sort_hi > 12) sort_hi = c - 1 - 12;
    while (sort_hi > 0 && (nsets << sort_hi) > (size_t)BIG_MAX_BINS) sort_hi--;
  }
  const int sort_lo = c - 1 - sort_hi;
  p.sort_hi = sort_hi, p.sort_lo = sort_lo;
  int idx_bits = 1;
  {
    const size_t max_idx = tab ? (size_t)nwin * in.tab_len : npts;
    while (((size_t)1 << idx_bits) < max_idx) idx_bits++;
  }
  p.idx_bits = idx_bits;
  const bool wide_fmt = p.wide_fmt = idx_bits + 1 + sort_lo > 32;
  const size_t nbl = p.nbl = (size_t)kwin << sort_hi;
  size_t stage_cap = 0;
  if (large) {
    const size_t fixed = 8 * nbl + 4 * (size_t)(sthr / 64) + 64;
    if (BIG_LDS_MAX > fixed) stage_cap = std::min(stage_max, (BIG_LDS_MAX - fixed) / (wide_fmt ? 8 : 6)) & ~(size_t)63;
  }
  p.stage_cap = stage_cap;
  const size_t tile_pts = p.tile_pts = (size_t)sthr * ppt;
  const bool big = p.big = npts * batch >= in.bigsort_min && sort_hi >= 1 && sort_lo >= 1 && sort_lo <= 12 &&
                           (nsets << sort_hi) <= (size_t)BIG_MAX_BINS &&
                           (large ? stage_cap >= (tab ? (size_t)nwin * tile_pts : tile_pts) : 8 * nbl <= BIG_LDS_MAX);
  p.wgroup = tab ? nwin : (int)std::min<size_t>((size_t)nwin, std::max<size_t>(1, stage_cap / tile_pts));
  const size_t nbins_tot = p.nbins_tot = nsets << sort_hi;
  // staged scatter: the histogram pass runs on the scatter's own tiles and hands over its per-tile counts (2 B per tile and
  // bin), so that the scatter does not walk the digits a third time
  p.tiles_big = ((npts + tile_pts - 1) / tile_pts) * batch;
  p.use_tcnt = big && large && tile_pts % BIG_THREADS == 0 && tile_pts < 65536;
  if (big) {
    // hist: 256-thread tiles of its own (any tiling of the points gives the same bin totals) unless it counts for the scatter
    p.hist_ppt = p.use_tcnt ? (int)(tile_pts / BIG_THREADS) : ppt;
    p.hist_lds = (nbins_tot + BIG_THREADS / 64) * 4;      // tile histogram (one vector's bins); all bins for the last workgroup's scan
    p.scatter_lds = large ? (2 * nbl + (size_t)(sthr / 64)) * 4 + stage_cap * (wide_fmt ? 8 : 6) : 2 * nbl * 4;
    p.binsort_lds = (2 * ((size_t)1 << sort_lo) + 1 + (size_t)(sthr / 64)) * 4 + (large ? (size_t)sthr * BIG_EPT * 6 : 0);
  }

  // ---- workspace layout: 256-byte aligned regions in the order of MsmRegionId
  size_t off = 0;
  auto take = [&](MsmRegionId id, size_t bytes) {
    p.r[id].off = off;
    p.r[id].bytes = bytes;
    off += (bytes + 255) & ~(size_t)255;
  };
  const size_t xyzz = 4 * (size_t)in.coord_bytes;
  take(R_COUNTS, nkeys * 4);
  take(R_HEAVY, msm_heavy_cap(nlanes) * 8 + 16);
  take(R_BINS, big ? msm_bins_words(nbins_tot) * 4 : 0);
  // ONE zeroing launch: the two-level sort writes every offset itself and needs the heavy-bucket counter, its bin counters
  // and the ticket zeroed (bins lies right behind the heavy list); the atomics sort its counts and the heavy-bucket counter
  // (the heavy list lies right behind the counts)
  p.zero_off = big ? p.r[R_HEAVY].off : p.r[R_COUNTS].off;
  p.zero_bytes = big ? p.r[R_BINS].off + (nbins_tot + 1) * 4 - p.zero_off : p.r[R_HEAVY].off + 16 - p.zero_off;
  take(R_CURSOR, nkeys * 4);
  take(R_OFFSETS, (nkeys + 1) * 4);
  take(R_BT, p.iscan_blocks * 4);
  take(R_SORTED, max_sorted * 4);
  take(R_K0, (size_t)nlanes * 4);                                // first bucket of every accumulate lane
  take(R_CANON, npts * batch * (size_t)in.scalar_bytes);         // canonical scalars (written by the first sort pass)
  if (big) {
    take(R_TMP, max_sorted * 4);
    if (wide_fmt) take(R_TMP_LO, max_sorted * 2);
    if (p.use_tcnt) take(R_TCNT, p.tiles_big * nbl * 2);
  }
  p.sort_region = off;
  p.ys = NS == 2 ? p.sort_region : 0;
  off = p.sort_region * NS;
  take(R_EDGE, NB * 2 * (size_t)nlanes * xyzz);                  // per base vector: head[nlanes], tail[nlanes]
  take(R_BUCKETS, NB * nkeys * xyzz);
  take(R_HPART, NB * (size_t)p.vcap * xyzz);                     // chunk sums of split heavy buckets
  take(R_RC, NB * nsets * p.red_groups * xyzz);
  p.ws_bytes = off;
  p.out_bytes = NB * nsets * p.nslices * xyzz;
  p.pinned_bytes = p.out_bytes + 64;

  p.fold.win = win;
  p.fold.kwin = kwin;
  p.fold.lo_bits = lo_bits;
  p.fold.tabbed = tab;
  p.fold.nb = (int)NB;
  p.fold.nsorts = (int)NS;
  p.fold.stats_off = p.out_bytes;
  p.fold.offered = npts * batch * NB * (size_t)nwin;
  p.fold.g2 = in.g2;
  return p;
}

// zk_msm_plan: [window bits, windows, sorted entries (= mixed additions) per accumulate lane, base-field multiplications
// per mixed addition] of a table-free MSM of one scalar vector over npts points
inline void msm_plan_of(MsmPlanIn in, int* out) {
  in.batch = 1, in.vectors = 1, in.tab_c = 0;
  const MsmPlan p = msm_plan(in);
  out[0] = p.win.c;
  out[1] = p.win.nwin;
  out[2] = (int)p.tmin;
  out[3] = in.g2 ? 28 : 10;
}

}  // namespace zk
