// Definitions of msm_launch / msm_table_launch (declared in msm.hpp).  Included ONLY by the msm_<curve>_g<k>.hip
// translation units, each of which instantiates them for one (scalar field, coordinate field) pair: the Pippenger
// kernels are the most expensive part of the build and compile in parallel this way.
#pragma once
#include "base_mul_few.hpp"
#include "msm.hpp"
#include "pack_split.hpp"

namespace zk {

#define MSM_HIP(x)                                           \
  do {                                                       \
    hipError_t _e = (x);                                     \
    if (_e != hipSuccess) return eng->hip_fail(_e, #x);      \
  } while (0)
// stage marker: with -DZK_MSM_DEBUG_SYNC (debug builds only) the stream is synchronised and checked after every stage
#ifdef ZK_MSM_DEBUG_SYNC
#define MSM_STAGE(name)                                                          \
  do {                                                                           \
    hipError_t _e = hipStreamSynchronize(st);                                    \
    fprintf(stderr, "[zk msm] %s done (%s) npts=%zu c=%d nwin=%d\n", name,       \
            hipGetErrorString(_e), pl.npts, pl.win.c, pl.win.nwin);              \
    if (_e != hipSuccess) return eng->hip_fail(_e, name);                        \
  } while (0)
#else
#define MSM_STAGE(name) do { } while (0)
#endif

// The arrays of a launch in the slot's workspace (msm_plan.hpp MsmRegionId) and its pinned buffer.  KF: the kernels' field
// type, same layout as the caller's.
template <class Fr, class KF>
struct MsmViews {
  uint32_t *counts, *heavy, *bins, *cursor, *offsets, *bt, *sorted, *k0, *tmp, *zero;
  uint16_t *tmp_lo, *tcnt;       // tcnt: nullptr unless the histogram counts for the staged scatter
  Fr* canon;
  XYZZ<KF>*edge, *buckets, *hpart, *rc;
  XYZZ<KF>* out;                 // the slices go straight to the slot's pinned host buffer (device-visible, coherent:
  uint32_t* stats;               // hipHostMalloc's default), the sorts' entry counts behind them
  MsmViews(const MsmPlan& pl, void* ws, void* pinned) {
    auto at = [&](MsmRegionId id) { return (char*)ws + pl.r[id].off; };
    counts = (uint32_t*)at(R_COUNTS), heavy = (uint32_t*)at(R_HEAVY), bins = (uint32_t*)at(R_BINS);
    cursor = (uint32_t*)at(R_CURSOR), offsets = (uint32_t*)at(R_OFFSETS), bt = (uint32_t*)at(R_BT);
    sorted = (uint32_t*)at(R_SORTED), k0 = (uint32_t*)at(R_K0), tmp = (uint32_t*)at(R_TMP);
    zero = (uint32_t*)((char*)ws + pl.zero_off);
    tmp_lo = (uint16_t*)at(R_TMP_LO), tcnt = pl.use_tcnt ? (uint16_t*)at(R_TCNT) : nullptr;
    canon = (Fr*)at(R_CANON);
    edge = (XYZZ<KF>*)at(R_EDGE), buckets = (XYZZ<KF>*)at(R_BUCKETS), hpart = (XYZZ<KF>*)at(R_HPART), rc = (XYZZ<KF>*)at(R_RC);
    out = (XYZZ<KF>*)pinned, stats = (uint32_t*)((char*)pinned + pl.out_bytes);
  }
};

// A launch with dynamic LDS: above the 48 KB every kernel may use, the kernel's limit is raised first (msm_lds_attr)
template <class... P, class... A>
hipError_t msm_launch_lds(int device, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  if (lds > 48 * 1024) {
    hipError_t e = msm_lds_attr((const void*)kernel, lds, device);
    if (e != hipSuccess) return e;
  }
  kernel<<<grid, block, lds, st>>>(args...);
  return hipSuccess;
}

// Stage 1: zero, then the sort (two-level or atomics) of the launch's digits into sorted[] / offsets[] / k0[]
template <class FrP, class KF>
int msm_stage_sort(IEngine* eng, const MsmPlan& pl, const MsmViews<Fp<FrP>, KF>& v, const MsmScalars<Fp<FrP>>& sc,
                   const Fp<FrP>* coef_d, size_t plen, const MsmBaseId& bid, const MsmScale1<Fp<FrP>>& sc1, hipStream_t st) {
  const size_t npts = pl.npts, ys = pl.ys, nkeys = pl.nkeys;
  const unsigned batch = (unsigned)pl.batch, NS = pl.nsorts;
  const int c = pl.win.c, nwin = pl.win.nwin, wide = pl.win.wide, sort_hi = pl.sort_hi, sort_lo = pl.sort_lo;
  MSM_HIP(msm_zero(v.zero, pl.zero_bytes, st, NS, ys));
  auto tiles = [&](size_t tile_pts) { return (unsigned)((npts + tile_pts - 1) / tile_pts); };      // per scalar vector
  ProfScope ps_(eng->prof, PROF_MSM_SORT, st, (double)npts * batch);
  if (pl.big) {
    const uint32_t wmask = pl.tabbed ? 0u : ~0u;
    const bool wf = pl.wide_fmt;
    {
      const unsigned tpv = tiles((size_t)BIG_THREADS * pl.hist_ppt);
      MSM_HIP(msm_launch_lds(eng->device, msm_hist_kernel<FrP>, dim3(tpv * batch, NS), dim3(BIG_THREADS), pl.hist_lds, st,
                             sc, coef_d, plen, c, nwin, wide, sort_hi, sort_lo, pl.hist_ppt, tpv, wmask, v.bins, bid, v.canon,
                             v.tcnt, ys, sc1));
    }
    if (pl.large) {
      const unsigned tpv = tiles(pl.tile_pts);
      // the points per thread are a template parameter of the staged scatter (its scalars live in registers): with a
      // table the whole tile is one round of nwin windows and the tile shrinks to fit the stage (ppt 4 / 2 / 1)
      auto* k = wf ? msm_scatter_kernel<FrP, 1024, BIG_PTS_PER_THREAD, true> : msm_scatter_kernel<FrP, 1024, BIG_PTS_PER_THREAD, false>;
      switch (pl.ppt) {
        case BIG_PTS_PER_THREAD: break;
        case 4: k = wf ? msm_scatter_kernel<FrP, 1024, 4, true> : msm_scatter_kernel<FrP, 1024, 4, false>; break;
        case 2: k = wf ? msm_scatter_kernel<FrP, 1024, 2, true> : msm_scatter_kernel<FrP, 1024, 2, false>; break;
        case 1: k = wf ? msm_scatter_kernel<FrP, 1024, 1, true> : msm_scatter_kernel<FrP, 1024, 1, false>; break;
        default: return eng->fail(ZK_ERR_GENERIC, "msm: unsupported scatter tile");
      }
      MSM_HIP(msm_launch_lds(eng->device, k, dim3(tpv * batch, NS), dim3(1024), pl.scatter_lds, st, sc, c, nwin, wide, sort_hi,
                             sort_lo, tpv, wmask, pl.wgroup, pl.pre_stride, pl.pre_off, pl.idx_bits, (uint32_t)pl.stage_cap,
                             v.bins, v.tmp, v.tmp_lo, v.canon, v.tcnt, ys));
    } else {
      const unsigned tpv = tiles((size_t)BIG_THREADS * pl.ppt);
      MSM_HIP(msm_launch_lds(eng->device, wf ? msm_scatter_direct_kernel<FrP, true> : msm_scatter_direct_kernel<FrP, false>,
                             dim3(tpv * batch, NS), dim3(BIG_THREADS), pl.scatter_lds, st, sc, c, nwin, wide, sort_hi, sort_lo,
                             pl.ppt, tpv, wmask, pl.pre_stride, pl.pre_off, pl.idx_bits, v.bins, v.tmp, v.tmp_lo, v.canon, ys));
    }
    auto* bk = pl.large ? (wf ? msm_binsort_kernel<1024, true, true> : msm_binsort_kernel<1024, false, true>)
                        : (wf ? msm_binsort_kernel<256, true, false> : msm_binsort_kernel<256, false, false>);
    MSM_HIP(msm_launch_lds(eng->device, bk, dim3((unsigned)pl.nbins_tot, NS), dim3((unsigned)pl.sthr), pl.binsort_lds, st, v.tmp,
                           v.tmp_lo, v.bins, (uint32_t)pl.nbins_tot, sort_hi, sort_lo, (uint32_t)(c - 1), pl.idx_bits,
                           (uint32_t)nkeys, pl.nlanes, pl.tmin, pl.cap, v.offsets, v.sorted, v.k0, ys));
    MSM_STAGE("big sort");
  } else {
    const dim3 pb(256), pgb((unsigned)((npts * batch + 255) / 256), NS);     // one thread per (scalar vector, point)
    const unsigned ib = (unsigned)pl.iscan_blocks;
    msm_digits_kernel<FrP, 0><<<pgb, pb, 0, st>>>(sc, coef_d, plen, c, nwin, wide, pl.pre_stride, pl.pre_off, v.counts, nullptr,
                                                 nullptr, bid, v.canon, ys, sc1);
    MSM_STAGE("digits/count");
    iscan_block_kernel<<<dim3(ib, NS), dim3(ISCAN_THREADS), 0, st>>>(v.counts, nkeys, v.bt, nullptr, nullptr, nullptr, 0, ys);
    iscan_carry_kernel<<<dim3(1, NS), dim3(ISCAN_THREADS), 0, st>>>(v.bt, pl.iscan_blocks, ys);
    iscan_block_kernel<<<dim3(ib, NS), dim3(ISCAN_THREADS), 0, st>>>(v.counts, nkeys, nullptr, v.bt, v.offsets, v.cursor, 1, ys);
    MSM_STAGE("scan");
    msm_lane_start_kernel<<<dim3((pl.nlanes + 255) / 256, NS), dim3(256), 0, st>>>(v.offsets, (uint32_t)nkeys, pl.nlanes, pl.tmin,
                                                                                 pl.cap, v.k0, ys);
    msm_digits_kernel<FrP, 1><<<pgb, pb, 0, st>>>(sc, coef_d, plen, c, nwin, wide, pl.pre_stride, pl.pre_off, nullptr, v.cursor,
                                                 v.sorted, bid, v.canon, ys, sc1);
  }
  return ZK_OK;
}

// Stage 2: the gates between the accumulate kernels of concurrent launches (msm.hpp MsmGate) and the accumulate kernel
template <class Fr, class Fld, class KF>
int msm_stage_accumulate(IEngine* eng, const MsmPlan& pl, const MsmViews<Fr, KF>& v, const MsmGate& gate, const void* bases,
                         const void* bases2, hipStream_t st) {
  constexpr bool G2FLD = IsExtField<Fld>::value;
  const unsigned NB = pl.vectors;
  const uint32_t nkeys = (uint32_t)pl.nkeys, nlanes = pl.nlanes;
  ProfScope ps_(eng->prof, G2FLD ? PROF_MSM_ACC_G2 : PROF_MSM_ACC_G1, st, (double)pl.npts * NB * pl.batch);
  if (gate.sorted_ev) {
    MSM_HIP(hipEventRecord(gate.sorted_ev, st));
    if (gate.sorted_cnt) gate.sorted_cnt->fetch_add(1, std::memory_order_release);
  }
  // the two host-side gates are bounded by the context's deadline (round 6): a launch that never comes -- the task that
  // would raise the flag failed before it, or never ran -- is an error with a name, not a spin for ever
  if (gate.n_wait_sorted) {
    if (!eng->spin_until([&] { return gate.sorted_cnt->load(std::memory_order_acquire) >= gate.sorted_need; }))
      return eng->fail(ZK_ERR_GENERIC, "msm launch: the sorts of the proof's other MSMs were not all enqueued within the deadline (" +
                                           std::to_string(gate.sorted_cnt->load()) + " of " + std::to_string(gate.sorted_need) + ")");
    for (int i = 0; i < gate.n_wait_sorted; i++) MSM_HIP(hipStreamWaitEvent(st, gate.wait_sorted[i], 0));
  }
  if (gate.wait_ev) {
    if (gate.wait_flag && !eng->spin_until([&] { return gate.wait_flag->load(std::memory_order_acquire) != 0; }))
      return eng->fail(ZK_ERR_GENERIC, "msm launch: the accumulate kernel ahead of this one in the batch's chain was not enqueued within the deadline");
    MSM_HIP(hipStreamWaitEvent(st, gate.wait_ev, 0));
  }
  if constexpr (G2FLD) {
    msm_accumulate_split_kernel<typename BaseParams<Fld>::type><<<dim3((nlanes + 31) / 32, NB), dim3(128), 0, st>>>(
        bases, bases2, v.sorted, v.offsets, nkeys, nlanes, pl.tmin, pl.cap, v.buckets, v.edge, v.heavy, v.k0, pl.ys);
  } else {
    msm_accumulate_kernel<KF><<<dim3((nlanes + 127) / 128, NB), dim3(128), 0, st>>>(
        (const Affine<KF>*)bases, (const Affine<KF>*)bases2, v.sorted, v.offsets, nkeys, nlanes, pl.tmin, pl.cap, v.buckets,
        v.edge, v.heavy, v.k0, pl.ys, 0);
  }
  if (gate.signal_ev) {
    MSM_HIP(hipEventRecord(gate.signal_ev, st));
    if (gate.signal_flag) gate.signal_flag->store(1, std::memory_order_release);
  }
  return ZK_OK;
}

// Stage 3: heavy buckets, finalize, reduce A and B (the bit slices land in the pinned buffer).  share (msm.hpp "SHARED
// BUCKET SET"): donated bucket arrays are added in the finalize kernel, behind their donors' events; base vectors
// [share->keep, vectors) of this launch donate theirs -- the reduction covers the vectors in front of them, if any.
template <class Fr, class Fld, class KF>
int msm_stage_reduce(IEngine* eng, const MsmPlan& pl, const MsmViews<Fr, KF>& v, hipStream_t st, const MsmShare<Fr>* share,
                     MsmPending* pend) {
  constexpr bool G2FLD = IsExtField<Fld>::value;
  const unsigned NB = pl.vectors, nsets = (unsigned)pl.nsets;
  const unsigned NR = share && share->keep >= 0 ? std::min<unsigned>((unsigned)share->keep, NB) : NB;      // vectors reduced here
  const uint32_t nkeys = (uint32_t)pl.nkeys, nlanes = pl.nlanes, tmin = pl.tmin, cap = pl.cap;
  const size_t ys = pl.ys;
  ProfScope ps_(eng->prof, G2FLD ? PROF_MSM_REDUCE_G2 : PROF_MSM_REDUCE, st, (double)pl.nkeys * NB);   // units: buckets
  const int qt = quad_threads(pl.batch > 1), qvl = qt / 4;
  const size_t quad_lds = (size_t)qvl * sizeof(XYZZ<Fld>);
  // buckets spread over many lanes (none for well-spread scalars: the workgroups read a zero count and leave)
  // (always one-wave workgroups: with 256 threads this launch, which normally reads one word and leaves, waited 90-150 us
  // for four free wave slots on one CU in a single proof's timeline)
  msm_heavy_kernel<KF><<<dim3(2048, NB), dim3(64), (size_t)16 * sizeof(XYZZ<Fld>), st>>>(v.edge, nlanes, tmin, cap, v.offsets, nkeys,
                                                                    v.buckets, v.heavy, v.hpart, pl.vcap, ys);
  MSM_STAGE("heavy buckets");
  MsmAbsorb<KF> ab{{nullptr, nullptr}};
  for (int i = 0; share && i < share->n_absorb; i++) {
    if (NB != 1 || i >= 2) return eng->fail(ZK_ERR_GENERIC, "msm launch: a launch over one base vector absorbs at most two bucket arrays");
    // a donor launched by another host thread: its pending launch is filled and its event recorded once the flag is up
    std::atomic<int>* fl = share->from_flag[i];
    if (fl && !eng->spin_until([&] { return fl->load(std::memory_order_acquire) != 0; }))
      return eng->fail(ZK_ERR_GENERIC, "msm launch: a launch that donates buckets to this one was not enqueued within the deadline");
    if (fl && fl->load(std::memory_order_acquire) < 0) return eng->fail(ZK_ERR_GENERIC, "msm launch: a launch that donates buckets to this one failed");
    const MsmPending* d = share->from[i];
    const void* arr = d ? d->donated[share->from_vec[i] & 1] : nullptr;
    if (!arr || !d->donated_ev || d->geo != pl.geo())
      return eng->fail(ZK_ERR_GENERIC, "msm launch: donated buckets of another geometry (the table registry changed between plan and launch?)");
    MSM_HIP(hipStreamWaitEvent(st, d->donated_ev, 0));
    ab.d[i] = (const XYZZ<KF>*)arr;
  }
  {
    // capped grid (grid-stride inside): enough one-wave workgroups to cover the chip a few times over
    const size_t fin_wgs = std::min<size_t>((pl.nkeys + FIN_THREADS / 4 - 1) / (FIN_THREADS / 4), 8192);
    // + workgroups that sum the chunk sums of split heavy buckets (they read the list's counter and leave, normally)
    const unsigned fin_extra = 256;
    msm_finalize_kernel<KF><<<dim3((unsigned)fin_wgs + fin_extra, NB), dim3(FIN_THREADS),
                              (size_t)(FIN_THREADS / 4) * sizeof(XYZZ<Fld>), st>>>(
        v.edge, nlanes, tmin, cap, v.offsets, nkeys, v.buckets, v.heavy, v.hpart, pl.vcap, (uint32_t)fin_wgs, ys, ab,
        // no reduce stage B in a launch that donates every vector: the sorts' entry counts leave from here
        NR == 0 ? v.stats : nullptr, pl.nsorts);
  }
  MSM_STAGE("finalize");
  if (NR < NB) {
    for (unsigned y = NR; y < NB; y++) pend->donated[y] = v.buckets + (size_t)y * nkeys;
    pend->donated_ev = share->donated_ev;
    pend->nred = (int)NR;
    if (share->donated_ev) MSM_HIP(hipEventRecord(share->donated_ev, st));
    if (NR == 0) return ZK_OK;
  }
  // quads per group: few groups (one bucket set) -> whole workgroups per group, shortest dependent chain; many groups
  // (one bucket set per window) -> 4 quads per group, waves stay full
  // As many quads per group as keep the whole launch resident at once (a second generation of workgroups doubles a
  // kernel that is one dependent chain): the chip holds 1024 SIMDs x (2 waves of the extension-field kernels, 3 of the
  // base-field ones) x 16 quads.
  const size_t tot_groups = (size_t)pl.red_groups * NR * nsets;
  const size_t tot_slices = (size_t)pl.nslices * NR * nsets;
  const size_t cap_quads = (size_t)1024 * (G2FLD ? 2 : 3) * 16;
  auto pick_nvl = [&](size_t groups) {
    int n = qvl;
    while (n > 4 && groups * (size_t)n > cap_quads) n >>= 1;
    return n;
  };
  const int nvl_a = pick_nvl(tot_groups), nvl_b = pick_nvl(tot_slices);
  const unsigned gpw_a = (unsigned)(qvl / nvl_a), gpw_b = (unsigned)(qvl / nvl_b);
  msm_reduce_a_kernel<KF><<<dim3((pl.red_groups + gpw_a - 1) / gpw_a, NR * nsets), dim3((unsigned)qt), quad_lds, st>>>(
      v.buckets, pl.B, pl.lo_bits, nvl_a, v.rc);
  msm_reduce_b_kernel<KF><<<dim3(((unsigned)pl.nslices + gpw_b - 1) / gpw_b, NR * nsets), dim3((unsigned)qt), quad_lds, st>>>(
      v.rc, pl.B, pl.lo_bits, nvl_b, v.out,
      // mixed additions actually performed = sorted entries (identity bases and zero digits leave none): one count per sort
      v.offsets + nkeys, ys, pl.nsorts, v.stats);
  return ZK_OK;
}

template <class FrP, class Fld>
int msm_launch(IEngine* eng, MsmSlot& slot, const MsmTuning& tune, const void* bases, const void* bases2,
               const void* scalars, size_t npts, const Fp<FrP>* coef_d, size_t part_len, hipStream_t st,
               MsmPending* pend, const MsmBatchArg* ba, const MsmShare<Fp<FrP>>* share) {
  using Fr = Fp<FrP>;
  using KF = typename KernelField<Fld>::type;     // same layout as Fld
  static_assert(sizeof(KF) == sizeof(Fld), "kernel field layout");
  static_assert(sizeof(XYZZ<Fld>) == 4 * sizeof(Fld), "the plan sizes XYZZ points as four coordinates");
  constexpr bool G2FLD = IsExtField<Fld>::value;
  *pend = MsmPending{};
  const unsigned NB = bases2 ? 2u : 1u;
  const void* const bases_in = bases;            // the caller's points (the identity test reads them, not the table rows)
  const void* const bases2_in = bases2;
  std::shared_ptr<const MsmTable> tab, tab2;
  const MsmPlan pl = msm_plan_for<FrP, Fld>(tune, bases, bases2, npts, ba ? (size_t)ba->nb : 1, share && share->scale1_on, &tab, &tab2);
  if (tab) bases = tab->data;
  if (tab2) bases2 = tab2->data;
  if (pl.err) return eng->fail(ZK_ERR_BAD_INPUT, pl.err);
  pend->fold = pl.fold;
  pend->geo = pl.geo();
  if (share && share->scale1_on && pl.nsorts != 2) return eng->fail(ZK_ERR_GENERIC, "msm launch: a scalar factor for the second base vector needs two vectors");
  if (share && share->keep >= 0 && pl.batch != 1) return eng->fail(ZK_ERR_GENERIC, "msm launch: a batched launch cannot donate buckets");
  if (npts == 0) {
    if (share && (share->n_absorb || share->keep >= 0)) return eng->fail(ZK_ERR_GENERIC, "msm launch: an empty launch shares no buckets");
    return ZK_OK;
  }
  hipError_t he = slot.ws.ensure(pl.ws_bytes);
  if (he != hipSuccess) return eng->hip_fail(he, "msm workspace");
  he = slot.ensure_pinned(pl.pinned_bytes);
  if (he != hipSuccess) return eng->hip_fail(he, "msm pinned buffer");
  if (!slot.ev) {
    he = hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming);
    if (he != hipSuccess) return eng->hip_fail(he, "msm event");
  }
  // From the first enqueue on the slot is busy and holds the tables; every exit records its event (a failed launch may
  // have enqueued work), so that only MsmSlot::wait frees it.
  slot.busy = true;
  slot.lent = share && share->keep >= 0 && (unsigned)share->keep < NB;
  slot.tab = tab;
  slot.tab2 = tab2;
  pend->slot = &slot;
  struct RecordOnExit {
    MsmSlot& s;
    hipStream_t st;
    bool done = false;
    ~RecordOnExit() {
      if (!done) (void)hipEventRecord(s.ev, st);
    }
  } record_on_exit{slot, st};
  const MsmViews<Fr, KF> v(pl, slot.ws.p, slot.pinned);
  MsmScalars<Fr> sc{};
  for (size_t b = 0; b < pl.batch; b++) sc.p[b] = (const Fr*)(ba ? ba->p[b] : scalars);
  sc.npts = (uint32_t)npts;
  sc.nb = (uint32_t)pl.batch;
  sc.sets_per = (uint32_t)pl.kwin;
  // identity bases: the first sort-stage kernel looks at the caller's points itself (msm.hpp MsmBaseId)
  MsmBaseId bid;
  if (!pl.no_identity) {
    bid.b0 = bases_in;
    bid.b1 = bases2_in;
    bid.elem16 = (uint32_t)(sizeof(Affine<KF>) / 16);
  }
  MsmScale1<Fr> sc1{};
  if (share && share->scale1_on) sc1.k = share->scale1, sc1.on = 1u;
  int rc = msm_stage_sort<FrP, KF>(eng, pl, v, sc, coef_d, part_len ? part_len : npts, bid, sc1, st);
  if (rc) return rc;
  MSM_STAGE("scatter");
  rc = msm_stage_accumulate<Fr, Fld, KF>(eng, pl, v, tune.gate, bases, bases2, st);
  if (rc) return rc;
  MSM_STAGE("accumulate");
  MsmShare<Fr> sh_ = share ? *share : MsmShare<Fr>{};
  if (sh_.keep >= 0 && !sh_.donated_ev) sh_.donated_ev = slot.ev;      // (then every vector donates: checked below)
  if (share && share->keep > 0 && !share->donated_ev) return eng->fail(ZK_ERR_GENERIC, "msm launch: a partial donor needs an event");
  rc = msm_stage_reduce<Fr, Fld, KF>(eng, pl, v, st, share ? &sh_ : nullptr, pend);
  if (rc) return rc;
  MSM_HIP(hipGetLastError());
  MSM_STAGE("reduce");
  MSM_HIP(hipEventRecord(slot.ev, st));
  record_on_exit.done = true;
  return ZK_OK;
}
#undef MSM_HIP
#undef MSM_STAGE

template <class FrP, class Fld>
int msm_table_launch(IEngine* eng, const void* bases, size_t len, int c, int nwin, int wide, void* table,
                     hipStream_t st) {
  using KF = typename KernelField<Fld>::type;
  msm_table_kernel<KF><<<dim3((unsigned)((len + 127) / 128)), dim3(128), 0, st>>>(
      (const Affine<KF>*)bases, len, c, nwin, wide, (Affine<KF>*)table);
  hipError_t he = hipGetLastError();
  if (he != hipSuccess) return eng->hip_fail(he, "msm_table_kernel");
  return ZK_OK;
}

template <class FrP, class Fld>
int pack_points_split_launch(IEngine* eng, const void* points, size_t nchunks, int n, const uint8_t* dig, int jlen,
                             const void* beta, void* shares, hipStream_t st) {
  if constexpr (IsExtField<Fld>::value) {
    using P = typename BaseParams<Fld>::type;
    Fp<P> b;
    memcpy(&b, beta, sizeof(b));
    pss_pack_points_jsf_split_kernel<FrP, P><<<dim3((unsigned)((nchunks * 4 + 127) / 128), (unsigned)n), dim3(128), 0, st>>>(
        (const Affine<Fp2<P>>*)points, nchunks, n, dig, jlen, b, (Affine<Fp2<P>>*)shares);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) return eng->hip_fail(he, "pss_pack_points_jsf_split_kernel");
    return ZK_OK;
  } else {
    return eng->fail(ZK_ERR_BAD_INPUT, "the quad-split pack kernel is for extension-field points");
  }
}

template <class FrP, class Fld>
int base_mul_split_launch(IEngine* eng, const void* scalars, size_t len, const void* table, int nwin, int wb, void* out,
                          hipStream_t st) {
  if constexpr (IsExtField<Fld>::value) {
    using P = typename BaseParams<Fld>::type;
    const dim3 grid((unsigned)((len * 4 + 127) / 128)), block(128);
    if (wb == 16)
      fixed_base_mul_split_kernel<FrP, P, 16><<<grid, block, 0, st>>>((const Fp<FrP>*)scalars, len, (const Affine<Fp2<P>>*)table,
                                                                      nwin, (Affine<Fp2<P>>*)out);
    else
      fixed_base_mul_split_kernel<FrP, P, 8><<<grid, block, 0, st>>>((const Fp<FrP>*)scalars, len, (const Affine<Fp2<P>>*)table,
                                                                     nwin, (Affine<Fp2<P>>*)out);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) return eng->hip_fail(he, "fixed_base_mul_split_kernel");
    return ZK_OK;
  } else {
    return eng->fail(ZK_ERR_BAD_INPUT, "the quad-split fixed-base kernel is for extension-field points");
  }
}

template <class FrP, class Fld>
int base_mul_few_launch(IEngine* eng, const void* scalars, size_t len, const void* table, int nwin, void* out, hipStream_t st) {
  using KF = typename KernelField<Fld>::type;
  if (!len) return ZK_OK;
  if (len > FEW_MAX_LEN || nwin > FEW_MAX_WIN) return eng->fail(ZK_ERR_BAD_INPUT, "base_mul_few: too many scalars or windows");
  base_mul_few_kernel<FrP, KF><<<dim3((unsigned)few_blocks(len)), dim3(FEW_BLOCK), 0, st>>>(
      (const Fp<FrP>*)scalars, len, (const Affine<KF>*)table, nwin, (Jacobian<KF>*)out);
  hipError_t he = hipGetLastError();
  if (he != hipSuccess) return eng->hip_fail(he, "base_mul_few_kernel");
  return ZK_OK;
}

#define ZK_INSTANTIATE_MSM(FRP, FLD)                                                                              \
  template int msm_launch<FRP, FLD>(IEngine*, MsmSlot&, const MsmTuning&, const void*, const void*, const void*, \
                                    size_t, const Fp<FRP>*, size_t, hipStream_t, MsmPending*, const MsmBatchArg*, \
                                    const MsmShare<Fp<FRP>>*);  \
  template int msm_table_launch<FRP, FLD>(IEngine*, const void*, size_t, int, int, int, void*, hipStream_t);     \
  template int pack_points_split_launch<FRP, FLD>(IEngine*, const void*, size_t, int, const uint8_t*, int, const void*, void*, hipStream_t); \
  template int base_mul_split_launch<FRP, FLD>(IEngine*, const void*, size_t, const void*, int, int, void*, hipStream_t); \
  template int base_mul_few_launch<FRP, FLD>(IEngine*, const void*, size_t, const void*, int, void*, hipStream_t);

}  // namespace zk
