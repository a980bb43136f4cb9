// Kernels and the host driver of the error-correcting unpack and the repair over packed scalar shares (gao.hpp says what
// they compute).  Included by gao_<curve>.hip only.  ONE driver, gao_run<FrP, REPAIR>, serves every public form from a
// GaoCall; each stage is ONE body and ONE kernel template, instantiated for the flag sets the forms need:
//   stage 1  one lane per chunk (two at l = 8): the n shares are loaded once, transformed in registers, coefficients k .. n - 1 tested; a
//            clean chunk gets its secrets (and message) and status 0, a dirty one is appended to a compact list
//   stage 2  one group of n lanes per listed chunk: Gao's decoder (gao_chunk) over the wave's cross-lane builtins.  Launched
//            unconditionally with a grid derived from nchunks; it reads the count from device memory, strides over the list and
//            leaves at once when the count is zero -- so the call never synchronises with the host.
// The flags: ER -- a party list with absent parties; SCAN (stage 1) / REPAIR (stage 2) -- the repair: stage 1 ends at the test
// of the coefficients, stage 2 stores lane p's re-encoding over the share of a party named in errpos, no secrets and no
// message; BATCH -- several words, one list; RANGE -- a word in a block with padding.
//   zk_pss_unpack_robust            -                 zk_pss_unpack_robust_parties      ER
//   zk_pss_repair                   REPAIR            zk_pss_repair_parties             ER REPAIR
//   zk_pss_repair_batch             REPAIR BATCH      zk_pss_repair_batch_parties       ER REPAIR BATCH
//   zk_pss_repair_range, all n      REPAIR RANGE      zk_pss_repair_range, a list       ER REPAIR RANGE
// and a list of all n parties is the form without ER.
#pragma once
#include <algorithm>

#include "engine.hpp"
#include "gao.hpp"

namespace zk {

constexpr int GAO_THREADS = 256;
// workgroups of stage 2 at most: 1024 x 4 waves are four waves per SIMD of the 256 CUs, all the decoder's ~100 registers
// allow to be useful; a longer dirty list is walked with a grid stride (crossed from 1024 * 256 / n + 1 dirty chunks on)
constexpr uint32_t GAO_STAGE2_GRID = 1024;

// ---------------------------------------------------------------- the device lane group: n consecutive lanes of a wave
struct GaoDevGroup {
  template <class T>
  using V = T;
  int n, p, base;          // lanes per group, this lane's index in its group, the wave lane of the group's lane 0
  template <class T>
  ZK_D const T& at(const T& v, int) const { return v; }
  template <class T, class Fn>
  ZK_D T make(Fn fn) const { return fn(p); }
  template <class T>
  ZK_D T bcast(const T& v, int src) const {
    T o;
#pragma unroll
    for (int i = 0; i < T::N; i++) o.v[i] = (uint32_t)__shfl((int)v.v[i], base + src, 64);
    return o;
  }
  template <class T>
  ZK_D T shift(const T& v, int d) const {
    const int s = p - d;
    T o;
#pragma unroll
    for (int i = 0; i < T::N; i++) {
      const uint32_t x = (uint32_t)__shfl((int)v.v[i], base + (s < 0 ? 0 : s), 64);
      o.v[i] = s < 0 ? 0u : x;
    }
    return o;
  }
  template <class Fn>
  ZK_D uint32_t ballot(Fn pred) const {
    const uint64_t m = __ballot(pred(p));
    return (uint32_t)(m >> base) & (n == 32 ? 0xffffffffu : (1u << n) - 1);
  }
  ZK_D bool wave_any(bool b) const { return __any(b) != 0; }
};

// Working memory: [0] number of dirty chunks; summary words when the caller passes none; the list of dirty chunks.
struct GaoWork {
  uint32_t* count;
  unsigned long long* summary;       // [3 + n]: clean, corrected, failed, corrections per party
  uint32_t* list;
};

// ---------------------------------------------------------------- the arguments of both kernels
// Filled once per call.  `ab` -- a kilobyte, read by stage 1 at compile-time indices -- is a member only with ER; every other
// member is a word or two.  Stage 2 takes the struct by value: its instances are register for register what they were with
// argument lists of their own (docs/gao_kernel_resources.md).  Stage 1 takes the members one by one (see its kernel).
struct GaoNone {};
template <class P, bool ER>
struct GaoArgs {
  using F = Fp<P>;
  GaoConsts<F> c;
  std::conditional_t<ER, GaoAbsentLoad<F>, GaoNone> ab;      // ER, stage 1
  const GaoAbsent<F>* tab;      // ER: the device table (stage 1 of the unpack, stage 2)
  const F* ilam;                // ER, REPAIR: the device table of the inverses
  int n, l;
  F* shares;                    // written by the repair only
  size_t item_stride;           // BATCH
  size_t nchunks;               // (RANGE: rg.cnt is read)
  GaoRangeDev rg;               // RANGE
  int k, rho;                   // the caller's dimension; ER: the number of absent parties
  uint32_t listed;              // ER: bit p -- party p is listed
  F* secrets;                   // the unpack
  F* message;
  uint8_t* status;
  uint32_t* errpos;
  GaoWork wk;
};

// ---------------------------------------------------------------- stage 1
// ER: the form with absent parties (gao.hpp): the shares are rows of the listed parties, multiplied by Lambda(w^p) as they are
// loaded -- ab by value, read at compile-time indices -- the word is tested and evaluated at dimension k + rho, a secret's last
// product is by 1 / (n Lambda(g w_2l^i)) and the message is deflated by the rho roots of Lambda.  tab: the device table.
// SCAN: the inverse transform and the test only -- status and errpos of a clean chunk, the list of the dirty ones, no secrets
// and no message: 1 / 5 / 17 products per chunk at l = 1, 2, 4; at l = 8 the two lanes' 17 each and the 15 of the split.
// SCAN with ER (zk_pss_repair_parties): listed -- bit p: party p is listed; its row is the number of listed parties below it.
// entry0: the list entry of this item's chunk 0 (gao_batch_entry; zk_pss_repair_batch), 0 for a single word.
// RANGE (with SCAN): the word lies in a block with padding (king_range.hpp GaoRange) -- nchunks is the count of valid columns,
// the rows are rg.stride apart, status and errpos are written at rg.chunk(column), the list holds columns.
template <class P, int L, bool ER, bool SCAN = false, bool RANGE = false>
__device__ __forceinline__ void gao_stage1_body(const GaoConsts<Fp<P>>& c, const Fp<P>* __restrict__ shares, size_t nchunks,
                                                int k, Fp<P>* __restrict__ secrets, Fp<P>* __restrict__ message,
                                                uint8_t* __restrict__ status, uint32_t* __restrict__ errpos, const GaoWork& wk,
                                                const GaoAbsentLoad<Fp<P>>* ab, int rho,
                                                const GaoAbsent<Fp<P>>* __restrict__ tab, uint32_t listed = 0,
                                                uint32_t entry0 = 0, [[maybe_unused]] const GaoRangeDev rg = GaoRangeDev{}) {
  using F = Fp<P>;
  static_assert(!RANGE || SCAN, "the range form is a repair");
  constexpr int N = 4 * L, SP = gao_split(L), M = N / SP;
  const size_t pitch = RANGE ? (size_t)rg.stride : nchunks;       // elements between two rows
  const int kd = ER ? k + rho : k;       // the dimension the word is tested and evaluated at
  __shared__ uint32_t wg_dirty, wg_base;
  if (threadIdx.x == 0) wg_dirty = 0;
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, j = t / SP;
  const int q = (int)(t % SP);
  const bool live = j < nchunks;         // (the SP lanes of a chunk are neighbours and agree)
  bool dirty = false;
  if (live) {
    F x[M];
    if constexpr (ER)
      gao_load<M, SP>(c, q, [&](int p) {
        if constexpr (SCAN) {      // the row from the list's bit mask, two scalar operations: 32 row numbers held in scalar
                                   // registers beside the constants made the l = 8 scan spill some
          const int row = __builtin_popcount(listed & ((1u << p) - 1));
          return (listed >> p) & 1 ? load_elem(shares + (size_t)row * pitch + j) * ab->lam[p] : F::zero();
        }
        const int row = ab->row[p];
        return row < 0 ? F::zero() : load_elem(shares + (size_t)row * pitch + j) * ab->lam[p];
      }, x);
    else
      gao_load<M, SP>(c, q, [&](int p) { return load_elem(shares + (size_t)p * pitch + j); }, x);
    gao_ifft<M, SP>(c, x);
    dirty = !gao_is_clean<M, SP>(x, kd, q);
    if (SP == 2) dirty = __shfl_xor((int)dirty, 1, 64) || dirty;
    if (!dirty) {
      if (q == 0) {
        const size_t sj = RANGE ? (size_t)rg.chunk((uint32_t)j) : j;
        status[sj] = 0;
        if (errpos) errpos[sj] = 0;
      }
      if constexpr (!SCAN) {
        auto put_message = [&](int i, const F& v) { store_elem(message + (size_t)i * nchunks + j, v); };
        auto put_secret = [&](int i, const F& v) {
          F sum = v;
          if (SP == 2) {           // the two lanes of the chunk are both here: add their parts
            F o;
#pragma unroll
            for (int w = 0; w < F::N; w++) o.v[w] = (uint32_t)__shfl_xor((int)v.v[w], 1, 64);
            sum = v + o;
          }
          if (q == 0) store_elem(secrets + j * L + i, sum);
        };
        if constexpr (!ER) {
          if (message) gao_clean_message<M, SP>(c, x, k, q, put_message);
          if (secrets) gao_clean_secrets<M, SP>(c, x, k, q, put_secret);
        } else {
          if (secrets) gao_clean_secrets<M, SP>(c, x, kd, q, [&](int i) { return tab->sscale[i]; }, put_secret);
          if (message) {             // x = n h Lambda -> n h, root by root (the secrets above needed h Lambda)
#pragma unroll 1
            for (int e = 0; e < rho; e++) {
              const F r = tab->root[e];
              gao_deflate<M, SP>(x, r, q, [&](int, const F& v) {
                F o;
#pragma unroll
                for (int w = 0; w < F::N; w++) o.v[w] = (uint32_t)__shfl_xor((int)v.v[w], 1, 64);
                return o;
              });
            }
            gao_clean_message<M, SP>(c, x, k, q, put_message);
          }
        }
      }
    }
  }
  if (q) dirty = false;                  // one entry per chunk
  // the dirty chunks of the wave take consecutive places: one LDS atomic per wave, one global atomic per workgroup
  const uint64_t m = __ballot(dirty);
  const uint32_t lane = threadIdx.x & 63, rank = (uint32_t)__popcll(m & (((uint64_t)1 << lane) - 1));
  uint32_t wave_off = 0;
  if (lane == 0 && m) wave_off = atomicAdd(&wg_dirty, (uint32_t)__popcll(m));
  wave_off = (uint32_t)__shfl((int)wave_off, 0, 64);
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t first = (size_t)blockIdx.x * (blockDim.x / SP);
    const uint32_t in_wg = (uint32_t)(nchunks - first < blockDim.x / SP ? nchunks - first : blockDim.x / SP);
    wg_base = wg_dirty ? atomicAdd(wk.count, wg_dirty) : 0;
    if (in_wg > wg_dirty) atomicAdd(wk.summary, (unsigned long long)(in_wg - wg_dirty));
  }
  __syncthreads();
  if (dirty) wk.list[wg_base + wave_off + rank] = entry0 + (uint32_t)j;
}
// BATCH: the scan of item blockIdx.y -- its matrix, its rows of status and errpos, its summary words; the count and the list
// are the batch's.  A flag the instance does not have hands the body the constant its form always had.
// The arguments are GaoArgs' members as PLAIN parameters, not the struct: a struct that holds pointers is passed as one value
// and loaded whole where the kernel begins, constants and load table included, while a parameter of its own is read where it
// is used (c, ab, rg) or re-read in place of a spill.  Taking the struct, the l = 8 scans spilled 44 to 88 scalar registers
// (10 and 2 this way) and the l = 8 ER SCAN RANGE instance lost a wave per SIMD over one AGPR; a parameter an instance does
// not name is never loaded and costs nothing.
template <class P, int L, bool ER, bool SCAN, bool RANGE, bool BATCH>
__global__ __launch_bounds__(GAO_THREADS) void gao_stage1_kernel(
    const GaoConsts<Fp<P>> c, const std::conditional_t<ER, GaoAbsentLoad<Fp<P>>, GaoNone> abv,
    const GaoAbsent<Fp<P>>* __restrict__ tab, const Fp<P>* __restrict__ shares, size_t item_stride, size_t nchunks_,
    const GaoRangeDev rg, int k, int rho, uint32_t listed, Fp<P>* __restrict__ secrets, Fp<P>* __restrict__ message,
    uint8_t* __restrict__ status, uint32_t* __restrict__ errpos, GaoWork wk) {
  static_assert(!BATCH || (SCAN && !RANGE), "a batch is a repair of whole words");
  size_t nchunks;
  if constexpr (RANGE) nchunks = rg.cnt;
  else nchunks = nchunks_;
  uint32_t entry0 = 0;
  if constexpr (BATCH) {
    const uint32_t item = blockIdx.y;
    wk.summary += (size_t)item * (3 + 4 * L);
    shares += item * item_stride, status += item * nchunks, errpos = errpos ? errpos + item * nchunks : nullptr;
    entry0 = gao_batch_entry(item, 0, (uint32_t)nchunks);
  }
  const GaoAbsentLoad<Fp<P>>* ab = nullptr;
  if constexpr (ER) ab = &abv;
  gao_stage1_body<P, L, ER, SCAN, RANGE>(c, shares, nchunks, k, SCAN ? nullptr : secrets, SCAN ? nullptr : message, status,
                                         errpos, wk, ab, ER ? rho : 0, ER && !SCAN ? tab : nullptr, ER && SCAN ? listed : 0u,
                                         entry0, RANGE ? rg : GaoRangeDev{});
}

// ---------------------------------------------------------------- stage 2
// ER: lane p reads its row and Lambda(w^p) from the device table (a run-time index: not from kernel arguments), the decoder
// runs at dimension k + rho and gao_absent_finish maps its result back to the listed shares
// REPAIR: `shares` is written: lane p stores its re-encoding h(w_n^p) when bit p of the final errpos is set; no secrets, no
// message (the decoder's flag RE).  With ER the store is h'(w^p) / Lambda(w^p) into the party's row; ilam: the device table of
// the inverses, read at a run-time index by a lane that stores
// BATCH (zk_pss_repair_batch): a list entry names (item, chunk) and is the chunk's index in status and errpos; the item's matrix
// is at shares + item * item_stride and its summary words at wk.summary + item * (3 + n), added to chunk by chunk -- the
// entries of a lane's walk belong to any items in any order.  With ER (zk_pss_repair_batch_parties) the item's matrix is the
// compact one of the party list: the load and the store address row `row` of it, the table is the same for every item
template <class P, bool REPAIR>
using GaoSharesPtr = std::conditional_t<REPAIR, Fp<P>*, const Fp<P>* __restrict__>;
template <class P>
struct GaoBatchItem {
  Fp<P>* sh;
  size_t chunk;
  unsigned long long* sum;
};
// RANGE (a repair, no batch): as in stage 1 -- a list entry is a column, the rows are rg.stride apart, status and errpos are
// written at rg.chunk(column)
template <class P, bool ER, bool REPAIR = false, bool BATCH = false, bool RANGE = false>
__device__ __forceinline__ void gao_stage2_body(const GaoConsts<Fp<P>>& c, int n, int l, GaoSharesPtr<P, REPAIR> shares,
                                                size_t nchunks, int k, Fp<P>* __restrict__ secrets,
                                                Fp<P>* __restrict__ message, uint8_t* __restrict__ status,
                                                uint32_t* __restrict__ errpos, const GaoWork& wk,
                                                const GaoAbsent<Fp<P>>* __restrict__ tab,
                                                const Fp<P>* __restrict__ ilam = nullptr, size_t item_stride = 0,
                                                [[maybe_unused]] const GaoRangeDev rg = GaoRangeDev{}) {
  using F = Fp<P>;
  static_assert(!BATCH || REPAIR, "a batch is a repair");
  static_assert(!RANGE || (REPAIR && !BATCH), "the range form is a repair of one word");
  const size_t pitch = RANGE ? (size_t)rg.stride : nchunks;       // elements between two rows of a single word
  const uint32_t cnt = *wk.count;
  const uint32_t gpb = GAO_THREADS / n, stride = gridDim.x * gpb;
  if (blockIdx.x * gpb >= cnt) return;
  const int p = threadIdx.x % n;
  const GaoDevGroup g{n, p, (int)(threadIdx.x & 63) / n * n};
  // this lane's points: w^p, w^-p and (lanes < l) g w_2l^p
  const F xp = gao_lane_pow<F, 5>(c.wpow2, p), xinv = gao_lane_pow<F, 5>(c.wipow2, p);
  const F sp = c.g * gao_lane_pow<F, 3>(c.spow2, p & 7);
  int kd = k, rho = 0, row = p;
  uint32_t listed = 0;
  F lam, slam, lamc;
  if constexpr (ER) {
    rho = tab->rho, kd = k + rho, listed = tab->listed, row = tab->ld.row[p];
    lam = tab->ld.lam[p], slam = tab->slam[p & 7], lamc = tab->lamc[p];
  }
  uint32_t n_fixed = 0, n_status1 = 0, n_status2 = 0;       // this lane's part of the summary, added once at the end
  for (uint32_t first = blockIdx.x * gpb; first < cnt; first += stride) {       // (uniform over the workgroup)
    const uint32_t gi = first + threadIdx.x / n;
    const bool live = gi < cnt;
    const size_t j = live ? wk.list[gi] : 0;       // BATCH: the entry -- the chunk's index in status and errpos
    // BATCH: the item's matrix, the chunk in it, the item's summary words
    [[maybe_unused]] const auto it = [&] {
      if constexpr (BATCH) {
        uint32_t item, chunk;
        gao_batch_decode((uint32_t)j, (uint32_t)nchunks, item, chunk);
        return GaoBatchItem<P>{shares + item * item_stride, chunk, wk.summary + (size_t)item * (3 + n)};
      } else {
        return 0;
      }
    }();
    F y;
    if constexpr (ER && BATCH) y = live && row >= 0 ? load_elem(it.sh + (size_t)row * nchunks + it.chunk) * lam : F::zero();
    else if constexpr (ER) y = live && row >= 0 ? load_elem(shares + (size_t)row * pitch + j) * lam : F::zero();
    else if constexpr (BATCH) y = live ? load_elem(it.sh + (size_t)p * nchunks + it.chunk) : F::zero();
    else y = live ? load_elem(shares + (size_t)p * pitch + j) : F::zero();
    GaoResult<F, GaoDevGroup, REPAIR> r = gao_chunk<F, GaoDevGroup, REPAIR>(g, c, n, kd, live, y, xp, xinv, sp);
    if constexpr (ER) gao_absent_finish<F, GaoDevGroup, REPAIR>(g, k, rho, listed, message != nullptr, slam, lamc, r);
    if (!live) continue;
    if constexpr (REPAIR && ER) {
      gao_repair_word_parties<F, GaoDevGroup>(
          g, r, [&](int) { return row; }, [&](int lane) { return load_elem(ilam + lane); },
          [&](int, int at, const F& v) {
            if constexpr (BATCH) store_elem(it.sh + (size_t)at * nchunks + it.chunk, v);
            else store_elem(shares + (size_t)at * pitch + j, v);
          });
    } else if constexpr (BATCH) {
      gao_repair_word<F, GaoDevGroup>(g, r, [&](int lane, const F& v) { store_elem(it.sh + (size_t)lane * nchunks + it.chunk, v); });
    } else if constexpr (REPAIR) {
      gao_repair_word<F, GaoDevGroup>(g, r, [&](int lane, const F& v) { store_elem(shares + (size_t)lane * pitch + j, v); });
    } else {
      if (message && p < k) store_elem(message + (size_t)p * nchunks + j, r.h);
      if (secrets && p < l) store_elem(secrets + j * l + p, r.sec);
    }
    if constexpr (BATCH) {
      if (p == 0) {
        status[j] = (uint8_t)r.status;
        if (errpos) errpos[j] = r.errpos;
        atomicAdd(it.sum + (r.status == 1 ? 1 : 2), 1ull);
      }
      if ((r.errpos >> p) & 1) atomicAdd(it.sum + 3 + p, 1ull);
      continue;
    }
    if (p == 0) {
      const size_t sj = RANGE ? (size_t)rg.chunk((uint32_t)j) : j;
      status[sj] = (uint8_t)r.status;
      if (errpos) errpos[sj] = r.errpos;
      if (r.status == 1) n_status1++;
      else n_status2++;
    }
    n_fixed += (r.errpos >> p) & 1;
  }
  if (n_status1) atomicAdd(wk.summary + 1, (unsigned long long)n_status1);
  if (n_status2) atomicAdd(wk.summary + 2, (unsigned long long)n_status2);
  if (n_fixed) atomicAdd(wk.summary + 3 + p, (unsigned long long)n_fixed);
}
template <class P, bool ER, bool REPAIR, bool BATCH, bool RANGE>
__global__ __launch_bounds__(GAO_THREADS) void gao_stage2_kernel(const GaoArgs<P, ER> a) {
  size_t nchunks;
  if constexpr (RANGE) nchunks = a.rg.cnt;
  else nchunks = a.nchunks;
  gao_stage2_body<P, ER, REPAIR, BATCH, RANGE>(a.c, a.n, a.l, a.shares, nchunks, a.k, REPAIR ? nullptr : a.secrets,
                                               REPAIR ? nullptr : a.message, a.status, a.errpos, a.wk, ER ? a.tab : nullptr,
                                               ER && REPAIR ? a.ilam : nullptr, BATCH ? a.item_stride : 0,
                                               RANGE ? a.rg : GaoRangeDev{});
}
// a table of a call (GaoAbsent, GaoInvLambda), from the launch's arguments to working memory: one word per lane
template <class T>
__global__ __launch_bounds__(GAO_THREADS) void gao_table_kernel(const T a, T* __restrict__ out) {
  static_assert(sizeof(T) % 4 == 0, "words");
  const uint32_t* src = (const uint32_t*)&a;
  uint32_t* dst = (uint32_t*)out;
  for (uint32_t i = threadIdx.x; i < sizeof(T) / 4; i += blockDim.x) dst[i] = src[i];
}

// ---------------------------------------------------------------- the host driver
#define GAO_HIP(expr)                                    \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return e->hip_fail(_e, #expr); \
  } while (0)

// fn(integral_constant<int, L>) for the packing factor l: the one place a run-time l becomes the kernels' L
template <class Fn>
int gao_with_l(IEngine* e, int l, Fn fn) {
  switch (l) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 8: return fn(std::integral_constant<int, 8>{});
    default: return e->fail(ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8");
  }
}

// A call that passed gao_call_check, with (ER) or without absent parties: one clear, with ER the table launches, stage 1 with
// the item on grid.y, stage 2 over the one list.  ids: the list as gao_list_check wrote it.
template <class FrP, bool REPAIR, bool ER>
int gao_launch(IEngine* e, void* wkp, int l, const GaoCall& call, const uint32_t* ids, hipStream_t st) {
  using Fr = Fp<FrP>;
  const int n = 4 * l;
  const size_t nchunks = call.nchunks, nitems = (size_t)call.nitems;
  const GaoLayout lay = gao_layout<Fr>(n, call.nitems, nchunks, ER, REPAIR);
  char* const wk = (char*)wkp;
  GaoArgs<FrP, ER> a{};
  a.c = gao_make_consts<FrP>(l);
  a.n = n, a.l = l, a.k = call.dimension;
  a.shares = (Fr*)call.shares, a.item_stride = call.item_stride, a.nchunks = nchunks;
  if (call.range) a.rg = gao_range_dev(*call.range);
  a.secrets = (Fr*)call.secrets, a.message = (Fr*)call.message, a.status = call.status, a.errpos = call.errpos;
  a.wk.count = (uint32_t*)wk;
  a.wk.summary = call.summary ? (unsigned long long*)call.summary : (unsigned long long*)(wk + 32);
  a.wk.list = (uint32_t*)(wk + lay.list);
  GAO_HIP(hipMemsetAsync(wk, 0, lay.tab, st));
  if (call.summary) GAO_HIP(hipMemsetAsync(call.summary, 0, nitems * (3 + n) * 8, st));
  const dim3 blk(GAO_THREADS);
  if constexpr (ER) {
    using Tab = GaoAbsent<Fr>;
    static_assert(sizeof(Tab) + 80 <= 4096 && sizeof(a) <= 4096, "the table and the arguments travel as kernel arguments");
    const Tab t = gao_make_absent<FrP>(a.c, l, ids, call.np, call.dimension);
    a.ab = t.ld, a.rho = t.rho, a.listed = t.listed, a.tab = (Tab*)(wk + lay.tab);
    gao_table_kernel<Tab><<<dim3(1), blk, 0, st>>>(t, (Tab*)(wk + lay.tab));
    if constexpr (REPAIR) {
      GaoInvLambda<Fr>* inv = (GaoInvLambda<Fr>*)(wk + lay.inv);
      a.ilam = inv->v;
      gao_table_kernel<GaoInvLambda<Fr>><<<dim3(1), blk, 0, st>>>(gao_make_inv_lambda<FrP>(t), inv);
    }
  }
  const size_t per_wg = GAO_THREADS / gao_split(l), gpb = GAO_THREADS / n;      // chunks per workgroup of stage 1, of stage 2
  const dim3 grid1((unsigned)((nchunks + per_wg - 1) / per_wg), (unsigned)nitems);
  const dim3 grid2((unsigned)std::min<size_t>((nitems * nchunks + gpb - 1) / gpb, GAO_STAGE2_GRID));
  // the kernels of one form: exactly the forms of the table at the head of this file are instantiated
  auto form = [&](auto range_, auto batch_) {
    constexpr bool RANGE = decltype(range_)::value, BATCH = decltype(batch_)::value;
    int rc = gao_with_l(e, l, [&](auto l_) {
      gao_stage1_kernel<FrP, decltype(l_)::value, ER, REPAIR, RANGE, BATCH><<<grid1, blk, 0, st>>>(
          a.c, a.ab, a.tab, a.shares, a.item_stride, a.nchunks, a.rg, a.k, a.rho, a.listed, a.secrets, a.message, a.status,
          a.errpos, a.wk);
      return (int)ZK_OK;
    });
    if (rc) return rc;
    gao_stage2_kernel<FrP, ER, REPAIR, BATCH, RANGE><<<grid2, blk, 0, st>>>(a);
    GAO_HIP(hipGetLastError());
    return (int)ZK_OK;
  };
  if constexpr (REPAIR) {
    if (call.range) return form(std::true_type{}, std::false_type{});
    if (call.batch()) return form(std::false_type{}, std::true_type{});
  }
  return form(std::false_type{}, std::false_type{});
}

template <class FrP, bool REPAIR>
int gao_run(IEngine* e, void* wk, int l, const GaoCall& call, hipStream_t st) {
  uint32_t ids[GAO_MAX_N];
  const GaoRefusal r = gao_call_check(l, call, REPAIR, ids);
  if (r.code) return e->fail(r.code, r.msg);
  if (call.nchunks == 0) {
    if (call.range && call.summary) GAO_HIP(hipMemsetAsync(call.summary, 0, (size_t)(3 + 4 * l) * 8, st));
    return ZK_OK;
  }
  return call.np == 4 * l ? gao_launch<FrP, REPAIR, false>(e, wk, l, call, ids, st)
                          : gao_launch<FrP, REPAIR, true>(e, wk, l, call, ids, st);
}
#undef GAO_HIP

}  // namespace zk
