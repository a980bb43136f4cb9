// Kernels and host drivers of zk_pss_unpack_robust, zk_pss_unpack_robust_parties, zk_pss_repair, zk_pss_repair_parties,
// zk_pss_repair_batch and zk_pss_repair_batch_parties (gao.hpp says what they compute).  Included
// by gao_<curve>.hip only.  Each stage is one body with two kernels: the all-parties one, and the one for a party list (ER).
//   stage 1  one lane per chunk (two at l = 8): the n shares are loaded once, transformed in registers, coefficients k .. n - 1 tested; a
//            clean chunk gets its secrets (and message) and status 0, a dirty one is appended to a compact list
//   stage 2  one group of n lanes per listed chunk: Gao's decoder (gao_chunk) over the wave's cross-lane builtins.  Launched
//            unconditionally with a grid derived from nchunks; it reads the count from device memory, strides over the list and
//            leaves at once when the count is zero -- so the call never synchronises with the host.
// zk_pss_repair is the all-parties form of both with no secrets and no message: stage 1 ends at the test of the coefficients
// (SCAN: the scan kernel), stage 2 stores lane p's re-encoding over the share of a party named in errpos (REPAIR).
// zk_pss_repair_parties is SCAN and REPAIR together with ER: the scan loads with the multiplication by Lambda(w^p) and tests
// at k + rho, the repair divides lane p's re-encoding by Lambda(w^p) again and stores it into the party's row.
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
template <class P, int L>
__global__ __launch_bounds__(GAO_THREADS) void gao_stage1_kernel(const GaoConsts<Fp<P>> c, const Fp<P>* __restrict__ shares,
                                                                size_t nchunks, int k, Fp<P>* __restrict__ secrets,
                                                                Fp<P>* __restrict__ message, uint8_t* __restrict__ status,
                                                                uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage1_body<P, L, false>(c, shares, nchunks, k, secrets, message, status, errpos, wk, nullptr, 0, nullptr);
}
template <class P, int L>
__global__ __launch_bounds__(GAO_THREADS) void gao_scan_kernel(const GaoConsts<Fp<P>> c, const Fp<P>* __restrict__ shares,
                                                              size_t nchunks, int k, uint8_t* __restrict__ status,
                                                              uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage1_body<P, L, false, true>(c, shares, nchunks, k, nullptr, nullptr, status, errpos, wk, nullptr, 0, nullptr);
}
template <class P, int L>
__global__ __launch_bounds__(GAO_THREADS) void gao_scan_parties_kernel(const GaoConsts<Fp<P>> c, const GaoAbsentLoad<Fp<P>> ab,
                                                                      const Fp<P>* __restrict__ shares, size_t nchunks, int k,
                                                                      int rho, uint32_t listed, uint8_t* __restrict__ status,
                                                                      uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage1_body<P, L, true, true>(c, shares, nchunks, k, nullptr, nullptr, status, errpos, wk, &ab, rho, nullptr, listed);
}
// the range forms of the two scans above (engine_dist.inc.hpp: a rank's [np][seg] block under the all-to-all king)
template <class P, int L>
__global__ __launch_bounds__(GAO_THREADS) void gao_scan_range_kernel(const GaoConsts<Fp<P>> c, const Fp<P>* __restrict__ shares,
                                                                    GaoRangeDev rg, int k, uint8_t* __restrict__ status,
                                                                    uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage1_body<P, L, false, true, true>(c, shares, rg.cnt, k, nullptr, nullptr, status, errpos, wk, nullptr, 0, nullptr, 0, 0,
                                           rg);
}
template <class P, int L>
__global__ __launch_bounds__(GAO_THREADS) void gao_scan_parties_range_kernel(
    const GaoConsts<Fp<P>> c, const GaoAbsentLoad<Fp<P>> ab, const Fp<P>* __restrict__ shares, GaoRangeDev rg, int k, int rho,
    uint32_t listed, uint8_t* __restrict__ status, uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage1_body<P, L, true, true, true>(c, shares, rg.cnt, k, nullptr, nullptr, status, errpos, wk, &ab, rho, nullptr, listed,
                                          0, rg);
}
// zk_pss_repair_batch: the scan of item blockIdx.y -- its matrix, its rows of status and errpos, its summary words; the count
// and the list are the batch's
template <class P, int L>
__global__ __launch_bounds__(GAO_THREADS) void gao_scan_batch_kernel(const GaoConsts<Fp<P>> c, const Fp<P>* __restrict__ shares,
                                                                    size_t item_stride, size_t nchunks, int k,
                                                                    uint8_t* __restrict__ status,
                                                                    uint32_t* __restrict__ errpos, GaoWork wk) {
  const uint32_t item = blockIdx.y;
  wk.summary += (size_t)item * (3 + 4 * L);
  gao_stage1_body<P, L, false, true>(c, shares + item * item_stride, nchunks, k, nullptr, nullptr, status + item * nchunks,
                                     errpos ? errpos + item * nchunks : nullptr, wk, nullptr, 0, nullptr, 0,
                                     gao_batch_entry(item, 0, (uint32_t)nchunks));
}
// zk_pss_repair_batch_parties: the scan of item blockIdx.y of a batch of compact matrices of one party list -- the load of
// gao_scan_parties_kernel (the row of party p is the popcount of `listed` below p), the item offsets and entry0 of the batch
template <class P, int L>
__global__ __launch_bounds__(GAO_THREADS) void gao_scan_batch_parties_kernel(
    const GaoConsts<Fp<P>> c, const GaoAbsentLoad<Fp<P>> ab, const Fp<P>* __restrict__ shares, size_t item_stride, size_t nchunks,
    int k, int rho, uint32_t listed, uint8_t* __restrict__ status, uint32_t* __restrict__ errpos, GaoWork wk) {
  const uint32_t item = blockIdx.y;
  wk.summary += (size_t)item * (3 + 4 * L);
  gao_stage1_body<P, L, true, true>(c, shares + item * item_stride, nchunks, k, nullptr, nullptr, status + item * nchunks,
                                    errpos ? errpos + item * nchunks : nullptr, wk, &ab, rho, nullptr, listed,
                                    gao_batch_entry(item, 0, (uint32_t)nchunks));
}
// k: the caller's dimension
template <class P, int L>
__global__ __launch_bounds__(GAO_THREADS) void gao_stage1_parties_kernel(
    const GaoConsts<Fp<P>> c, const GaoAbsentLoad<Fp<P>> ab, const GaoAbsent<Fp<P>>* __restrict__ tab,
    const Fp<P>* __restrict__ shares, size_t nchunks, int k, int rho, Fp<P>* __restrict__ secrets, Fp<P>* __restrict__ message,
    uint8_t* __restrict__ status, uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage1_body<P, L, true>(c, shares, nchunks, k, secrets, message, status, errpos, wk, &ab, rho, tab);
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
template <class P>
__global__ __launch_bounds__(GAO_THREADS) void gao_stage2_kernel(const GaoConsts<Fp<P>> c, int n, int l,
                                                                const Fp<P>* __restrict__ shares, size_t nchunks, int k,
                                                                Fp<P>* __restrict__ secrets, Fp<P>* __restrict__ message,
                                                                uint8_t* __restrict__ status, uint32_t* __restrict__ errpos,
                                                                GaoWork wk) {
  gao_stage2_body<P, false>(c, n, l, shares, nchunks, k, secrets, message, status, errpos, wk, nullptr);
}
template <class P>
__global__ __launch_bounds__(GAO_THREADS) void gao_repair_kernel(const GaoConsts<Fp<P>> c, int n, int l, Fp<P>* shares,
                                                                size_t nchunks, int k, uint8_t* __restrict__ status,
                                                                uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage2_body<P, false, true>(c, n, l, shares, nchunks, k, nullptr, nullptr, status, errpos, wk, nullptr);
}
template <class P>
__global__ __launch_bounds__(GAO_THREADS) void gao_repair_batch_kernel(const GaoConsts<Fp<P>> c, int n, int l, Fp<P>* shares,
                                                                      size_t item_stride, size_t nchunks, int k,
                                                                      uint8_t* __restrict__ status,
                                                                      uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage2_body<P, false, true, true>(c, n, l, shares, nchunks, k, nullptr, nullptr, status, errpos, wk, nullptr, nullptr,
                                        item_stride);
}
// the range forms of gao_repair_kernel and gao_repair_parties_kernel
template <class P>
__global__ __launch_bounds__(GAO_THREADS) void gao_repair_range_kernel(const GaoConsts<Fp<P>> c, int n, int l, Fp<P>* shares,
                                                                      GaoRangeDev rg, int k, uint8_t* __restrict__ status,
                                                                      uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage2_body<P, false, true, false, true>(c, n, l, shares, rg.cnt, k, nullptr, nullptr, status, errpos, wk, nullptr, nullptr,
                                               0, rg);
}
template <class P>
__global__ __launch_bounds__(GAO_THREADS) void gao_repair_parties_range_kernel(
    const GaoConsts<Fp<P>> c, const GaoAbsent<Fp<P>>* __restrict__ tab, const Fp<P>* __restrict__ ilam, int n, int l,
    Fp<P>* shares, GaoRangeDev rg, int k, uint8_t* __restrict__ status, uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage2_body<P, true, true, false, true>(c, n, l, shares, rg.cnt, k, nullptr, nullptr, status, errpos, wk, tab, ilam, 0, rg);
}
// k: the caller's dimension
template <class P>
__global__ __launch_bounds__(GAO_THREADS) void gao_stage2_parties_kernel(
    const GaoConsts<Fp<P>> c, const GaoAbsent<Fp<P>>* __restrict__ tab, int n, int l, const Fp<P>* __restrict__ shares,
    size_t nchunks, int k, Fp<P>* __restrict__ secrets, Fp<P>* __restrict__ message, uint8_t* __restrict__ status,
    uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage2_body<P, true>(c, n, l, shares, nchunks, k, secrets, message, status, errpos, wk, tab);
}
template <class P>
__global__ __launch_bounds__(GAO_THREADS) void gao_repair_parties_kernel(const GaoConsts<Fp<P>> c,
                                                                        const GaoAbsent<Fp<P>>* __restrict__ tab,
                                                                        const Fp<P>* __restrict__ ilam, int n, int l,
                                                                        Fp<P>* shares, size_t nchunks, int k,
                                                                        uint8_t* __restrict__ status,
                                                                        uint32_t* __restrict__ errpos, GaoWork wk) {
  gao_stage2_body<P, true, true>(c, n, l, shares, nchunks, k, nullptr, nullptr, status, errpos, wk, tab, ilam);
}
template <class P>
__global__ __launch_bounds__(GAO_THREADS) void gao_repair_batch_parties_kernel(
    const GaoConsts<Fp<P>> c, const GaoAbsent<Fp<P>>* __restrict__ tab, const Fp<P>* __restrict__ ilam, int n, int l,
    Fp<P>* shares, size_t item_stride, size_t nchunks, int k, uint8_t* __restrict__ status, uint32_t* __restrict__ errpos,
    GaoWork wk) {
  gao_stage2_body<P, true, true, true>(c, n, l, shares, nchunks, k, nullptr, nullptr, status, errpos, wk, tab, ilam, item_stride);
}
// the table of a call, from the launch's arguments to working memory: one word per lane
template <class F>
__global__ __launch_bounds__(GAO_THREADS) void gao_absent_table_kernel(const GaoAbsent<F> a, GaoAbsent<F>* __restrict__ out) {
  static_assert(sizeof(GaoAbsent<F>) % 4 == 0, "words");
  const uint32_t* src = (const uint32_t*)&a;
  uint32_t* dst = (uint32_t*)out;
  for (uint32_t i = threadIdx.x; i < sizeof(GaoAbsent<F>) / 4; i += blockDim.x) dst[i] = src[i];
}

// the same for the inverses of a repair with a party list
template <class F>
__global__ __launch_bounds__(GAO_THREADS) void gao_inv_lambda_table_kernel(const GaoInvLambda<F> a, GaoInvLambda<F>* __restrict__ out) {
  static_assert(sizeof(GaoInvLambda<F>) % 4 == 0, "words");
  const uint32_t* src = (const uint32_t*)&a;
  uint32_t* dst = (uint32_t*)out;
  for (uint32_t i = threadIdx.x; i < sizeof(GaoInvLambda<F>) / 4; i += blockDim.x) dst[i] = src[i];
}

// ---------------------------------------------------------------- host driver
#define GAO_HIP(expr)                                    \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return e->hip_fail(_e, #expr); \
  } while (0)

// REPAIR: zk_pss_repair -- the scan in place of stage 1, the repair form of stage 2, `shares` written
template <class FrP, bool REPAIR>
int gao_all_parties_run(IEngine* e, DevBuf& wkbuf, int l, std::conditional_t<REPAIR, void*, const void*> shares, size_t nchunks,
                        int dimension, void* secrets, void* message, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                        hipStream_t st, const GaoRange* rg = nullptr) {
  using Fr = Fp<FrP>;
  const int n = 4 * l;
  if (dimension < 1 || dimension > n - 1) return e->fail(ZK_ERR_BAD_INPUT, "dimension must lie in 1 .. n - 1");
  if (rg && !REPAIR) return e->fail(ZK_ERR_BAD_INPUT, "the range form is a repair");
  if (nchunks == 0) return ZK_OK;
  if (!shares || !status) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
  if (nchunks >= ((size_t)1 << 32)) return e->fail(ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks");
  constexpr size_t head = 320;                                       // the count, then the summary words from byte 32 on
  static_assert(32 + (3 + GAO_MAX_N) * 8 <= head && head % 32 == 0, "layout");
  GAO_HIP(wkbuf.ensure(head + nchunks * 4));
  GaoWork wk;
  wk.count = (uint32_t*)wkbuf.p;
  wk.summary = summary ? (unsigned long long*)summary : (unsigned long long*)((char*)wkbuf.p + 32);
  wk.list = (uint32_t*)((char*)wkbuf.p + head);
  GAO_HIP(hipMemsetAsync(wkbuf.p, 0, head, st));
  if (summary) GAO_HIP(hipMemsetAsync(summary, 0, (size_t)(3 + n) * 8, st));
  const GaoConsts<Fr> c = gao_make_consts<FrP>(l);
  const size_t per_wg = GAO_THREADS / gao_split(l);                  // chunks per workgroup of stage 1
  const dim3 blk(GAO_THREADS), grid1((unsigned)((nchunks + per_wg - 1) / per_wg));
  std::conditional_t<REPAIR, Fr*, const Fr*> sh = (decltype(sh))shares;
  Fr* sec = (Fr*)secrets;
  Fr* msg = (Fr*)message;
  if constexpr (REPAIR) {
    if (rg) {      // the word in a block with padding: nchunks is rg->cnt (gao_repair_range_run)
      const GaoRangeDev rd = gao_range_dev(*rg);
      switch (l) {
        case 1: gao_scan_range_kernel<FrP, 1><<<grid1, blk, 0, st>>>(c, sh, rd, dimension, status, errpos, wk); break;
        case 2: gao_scan_range_kernel<FrP, 2><<<grid1, blk, 0, st>>>(c, sh, rd, dimension, status, errpos, wk); break;
        case 4: gao_scan_range_kernel<FrP, 4><<<grid1, blk, 0, st>>>(c, sh, rd, dimension, status, errpos, wk); break;
        case 8: gao_scan_range_kernel<FrP, 8><<<grid1, blk, 0, st>>>(c, sh, rd, dimension, status, errpos, wk); break;
        default: return e->fail(ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8");
      }
      const size_t gpb_r = GAO_THREADS / n;
      const dim3 grid_r((unsigned)std::min<size_t>((nchunks + gpb_r - 1) / gpb_r, GAO_STAGE2_GRID));
      gao_repair_range_kernel<FrP><<<grid_r, blk, 0, st>>>(c, n, l, sh, rd, dimension, status, errpos, wk);
      GAO_HIP(hipGetLastError());
      return ZK_OK;
    }
  }
  if constexpr (REPAIR) switch (l) {
    case 1: gao_scan_kernel<FrP, 1><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, status, errpos, wk); break;
    case 2: gao_scan_kernel<FrP, 2><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, status, errpos, wk); break;
    case 4: gao_scan_kernel<FrP, 4><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, status, errpos, wk); break;
    case 8: gao_scan_kernel<FrP, 8><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, status, errpos, wk); break;
    default: return e->fail(ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8");
  }
  else switch (l) {
    case 1: gao_stage1_kernel<FrP, 1><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, sec, msg, status, errpos, wk); break;
    case 2: gao_stage1_kernel<FrP, 2><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, sec, msg, status, errpos, wk); break;
    case 4: gao_stage1_kernel<FrP, 4><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, sec, msg, status, errpos, wk); break;
    case 8: gao_stage1_kernel<FrP, 8><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, sec, msg, status, errpos, wk); break;
    default: return e->fail(ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8");
  }
  const size_t gpb = GAO_THREADS / n;
  const dim3 grid2((unsigned)std::min<size_t>((nchunks + gpb - 1) / gpb, GAO_STAGE2_GRID));
  if constexpr (REPAIR) gao_repair_kernel<FrP><<<grid2, blk, 0, st>>>(c, n, l, sh, nchunks, dimension, status, errpos, wk);
  else gao_stage2_kernel<FrP><<<grid2, blk, 0, st>>>(c, n, l, sh, nchunks, dimension, sec, msg, status, errpos, wk);
  GAO_HIP(hipGetLastError());
  return ZK_OK;
}
template <class FrP>
int gao_unpack_robust_run(IEngine* e, DevBuf& wkbuf, int l, const void* shares, size_t nchunks, int dimension, void* secrets,
                          void* message, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) {
  return gao_all_parties_run<FrP, false>(e, wkbuf, l, shares, nchunks, dimension, secrets, message, status, errpos, summary, st);
}
template <class FrP>
int gao_repair_run(IEngine* e, DevBuf& wkbuf, int l, void* shares, size_t nchunks, int dimension, uint8_t* status,
                   uint32_t* errpos, uint64_t* summary, hipStream_t st) {
  return gao_all_parties_run<FrP, true>(e, wkbuf, l, shares, nchunks, dimension, nullptr, nullptr, status, errpos, summary, st);
}
// zk_pss_repair_batch: one clear, one scan with the item on grid.y, one repair launch over the one list of all items
template <class FrP>
int gao_repair_batch_run(IEngine* e, void* wkp, int l, void* shares, size_t item_stride, int nitems, size_t nchunks,
                         int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) {
  using Fr = Fp<FrP>;
  const int n = 4 * l;
  const size_t head = gao_batch_head(n, nitems);
  GaoWork wk;
  wk.count = (uint32_t*)wkp;
  wk.summary = summary ? (unsigned long long*)summary : (unsigned long long*)((char*)wkp + 32);
  wk.list = (uint32_t*)((char*)wkp + head);
  GAO_HIP(hipMemsetAsync(wkp, 0, head, st));
  if (summary) GAO_HIP(hipMemsetAsync(summary, 0, (size_t)nitems * (3 + n) * 8, st));
  const GaoConsts<Fr> c = gao_make_consts<FrP>(l);
  const size_t per_wg = GAO_THREADS / gao_split(l);
  const dim3 blk(GAO_THREADS), grid1((unsigned)((nchunks + per_wg - 1) / per_wg), (unsigned)nitems);
  Fr* sh = (Fr*)shares;
  switch (l) {
    case 1: gao_scan_batch_kernel<FrP, 1><<<grid1, blk, 0, st>>>(c, sh, item_stride, nchunks, dimension, status, errpos, wk); break;
    case 2: gao_scan_batch_kernel<FrP, 2><<<grid1, blk, 0, st>>>(c, sh, item_stride, nchunks, dimension, status, errpos, wk); break;
    case 4: gao_scan_batch_kernel<FrP, 4><<<grid1, blk, 0, st>>>(c, sh, item_stride, nchunks, dimension, status, errpos, wk); break;
    case 8: gao_scan_batch_kernel<FrP, 8><<<grid1, blk, 0, st>>>(c, sh, item_stride, nchunks, dimension, status, errpos, wk); break;
    default: return e->fail(ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8");
  }
  const size_t gpb = GAO_THREADS / n, total = (size_t)nitems * nchunks;
  const dim3 grid2((unsigned)std::min<size_t>((total + gpb - 1) / gpb, GAO_STAGE2_GRID));
  gao_repair_batch_kernel<FrP><<<grid2, blk, 0, st>>>(c, n, l, sh, item_stride, nchunks, dimension, status, errpos, wk);
  GAO_HIP(hipGetLastError());
  return ZK_OK;
}
// zk_pss_repair_batch_parties: the launches of the batch above with the two tables of the party list put into working memory
// ahead of them, once per call: one clear, GaoAbsent, GaoInvLambda, one scan with the item on grid.y, one repair launch over
// the one list.  ids: np ascending party ids below n, dimension < np < n (the caller's checks; np == n is the batch above).
template <class FrP>
int gao_repair_batch_parties_run(IEngine* e, void* wkp, int l, void* shares, const uint32_t* ids, int np, size_t item_stride,
                                 int nitems, size_t nchunks, int dimension, uint8_t* status, uint32_t* errpos,
                                 uint64_t* summary, hipStream_t st) {
  using Fr = Fp<FrP>;
  using Tab = GaoAbsent<Fr>;
  const int n = 4 * l;
  static_assert(sizeof(Tab) + 80 <= 4096, "the table travels as a kernel argument");
  const GaoBatchPartiesWork lay = gao_batch_parties_work<Fr>(n, nitems, nchunks);
  GaoWork wk;
  wk.count = (uint32_t*)wkp;
  wk.summary = summary ? (unsigned long long*)summary : (unsigned long long*)((char*)wkp + 32);
  wk.list = (uint32_t*)((char*)wkp + lay.list);
  Tab* tab = (Tab*)((char*)wkp + lay.tab);
  GaoInvLambda<Fr>* inv = (GaoInvLambda<Fr>*)((char*)wkp + lay.inv);
  GAO_HIP(hipMemsetAsync(wkp, 0, lay.tab, st));
  if (summary) GAO_HIP(hipMemsetAsync(summary, 0, (size_t)nitems * (3 + n) * 8, st));
  const GaoConsts<Fr> c = gao_make_consts<FrP>(l);
  const Tab a = gao_make_absent<FrP>(c, l, ids, np, dimension);
  const dim3 blk(GAO_THREADS);
  gao_absent_table_kernel<Fr><<<dim3(1), blk, 0, st>>>(a, tab);
  gao_inv_lambda_table_kernel<Fr><<<dim3(1), blk, 0, st>>>(gao_make_inv_lambda<FrP>(a), inv);
  const size_t per_wg = GAO_THREADS / gao_split(l);
  const dim3 grid1((unsigned)((nchunks + per_wg - 1) / per_wg), (unsigned)nitems);
  Fr* sh = (Fr*)shares;
  const int k = dimension, rho = a.rho;
  switch (l) {
    case 1: gao_scan_batch_parties_kernel<FrP, 1><<<grid1, blk, 0, st>>>(c, a.ld, sh, item_stride, nchunks, k, rho, a.listed, status, errpos, wk); break;
    case 2: gao_scan_batch_parties_kernel<FrP, 2><<<grid1, blk, 0, st>>>(c, a.ld, sh, item_stride, nchunks, k, rho, a.listed, status, errpos, wk); break;
    case 4: gao_scan_batch_parties_kernel<FrP, 4><<<grid1, blk, 0, st>>>(c, a.ld, sh, item_stride, nchunks, k, rho, a.listed, status, errpos, wk); break;
    case 8: gao_scan_batch_parties_kernel<FrP, 8><<<grid1, blk, 0, st>>>(c, a.ld, sh, item_stride, nchunks, k, rho, a.listed, status, errpos, wk); break;
    default: return e->fail(ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8");
  }
  const size_t gpb = GAO_THREADS / n, total = (size_t)nitems * nchunks;
  const dim3 grid2((unsigned)std::min<size_t>((total + gpb - 1) / gpb, GAO_STAGE2_GRID));
  gao_repair_batch_parties_kernel<FrP><<<grid2, blk, 0, st>>>(c, tab, inv->v, n, l, sh, item_stride, nchunks, k, status, errpos, wk);
  GAO_HIP(hipGetLastError());
  return ZK_OK;
}
// With all n parties listed this is the call above; otherwise the kernels' forms for absent parties, with the table of the
// party list (gao_make_absent, host) put into working memory by a launch of its own ahead of them.
// REPAIR: zk_pss_repair_parties -- the scan in place of stage 1, the repair form of stage 2, `shares` written; the inverses
// 1 / Lambda(w^p) go into a second table behind the first, by a launch of their own.
template <class FrP, bool REPAIR>
int gao_party_list_run(IEngine* e, DevBuf& wkbuf, int l, std::conditional_t<REPAIR, void*, const void*> shares,
                       const uint32_t* parties, int np, size_t nchunks, int dimension, void* secrets, void* message,
                       uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st, const GaoRange* rg = nullptr) {
  using Fr = Fp<FrP>;
  const int n = 4 * l;
  if (l != 1 && l != 2 && l != 4 && l != 8) return e->fail(ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8");
  if (np <= 0 || np > n) return e->fail(ZK_ERR_BAD_INPUT, "bad party count");
  if (rg && !REPAIR) return e->fail(ZK_ERR_BAD_INPUT, "the range form is a repair");
  uint32_t ids[GAO_MAX_N];
  for (int i = 0; i < np; i++) {
    ids[i] = parties ? parties[i] : (uint32_t)i;
    if (ids[i] >= (uint32_t)n || (i > 0 && ids[i] <= ids[i - 1]))
      return e->fail(ZK_ERR_BAD_INPUT, "party ids must be ascending and < n");
  }
  if (dimension < 1 || dimension > n - 1) return e->fail(ZK_ERR_BAD_INPUT, "dimension must lie in 1 .. n - 1");
  if (np <= dimension) return e->fail(ZK_ERR_PROTOCOL, "Not enough shares to reconstruct");      // pss.rs:183-186
  if (np == n)
    return gao_all_parties_run<FrP, REPAIR>(e, wkbuf, l, shares, nchunks, dimension, secrets, message, status, errpos, summary,
                                            st, rg);
  if (nchunks == 0) return ZK_OK;
  if (!shares || !status) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
  if (nchunks >= ((size_t)1 << 32)) return e->fail(ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks");
  using Tab = GaoAbsent<Fr>;
  constexpr size_t head = 320, tab_bytes = (sizeof(Tab) + 31) / 32 * 32;      // count, summary words, then the table
  static_assert(sizeof(Tab) + 64 <= 4096, "the table travels as a kernel argument");
  constexpr size_t inv_bytes = REPAIR ? sizeof(GaoInvLambda<Fr>) : 0;
  static_assert(inv_bytes % 32 == 0, "the list stays aligned");
  GAO_HIP(wkbuf.ensure(head + tab_bytes + inv_bytes + nchunks * 4));
  GaoWork wk;
  wk.count = (uint32_t*)wkbuf.p;
  wk.summary = summary ? (unsigned long long*)summary : (unsigned long long*)((char*)wkbuf.p + 32);
  wk.list = (uint32_t*)((char*)wkbuf.p + head + tab_bytes + inv_bytes);
  Tab* tab = (Tab*)((char*)wkbuf.p + head);
  GAO_HIP(hipMemsetAsync(wkbuf.p, 0, head, st));
  if (summary) GAO_HIP(hipMemsetAsync(summary, 0, (size_t)(3 + n) * 8, st));
  const GaoConsts<Fr> c = gao_make_consts<FrP>(l);
  const Tab a = gao_make_absent<FrP>(c, l, ids, np, dimension);
  const dim3 blk(GAO_THREADS);
  gao_absent_table_kernel<Fr><<<dim3(1), blk, 0, st>>>(a, tab);
  [[maybe_unused]] GaoInvLambda<Fr>* inv = (GaoInvLambda<Fr>*)((char*)wkbuf.p + head + tab_bytes);
  if constexpr (REPAIR) gao_inv_lambda_table_kernel<Fr><<<dim3(1), blk, 0, st>>>(gao_make_inv_lambda<FrP>(a), inv);
  const size_t per_wg = GAO_THREADS / gao_split(l);
  const dim3 grid1((unsigned)((nchunks + per_wg - 1) / per_wg));
  std::conditional_t<REPAIR, Fr*, const Fr*> sh = (decltype(sh))shares;
  Fr* sec = (Fr*)secrets;
  Fr* msg = (Fr*)message;
  const int k = dimension, rho = a.rho;
  if constexpr (REPAIR) {
    if (rg) {      // the word in a block with padding: nchunks is rg->cnt (gao_repair_range_run)
      const GaoRangeDev rd = gao_range_dev(*rg);
      switch (l) {
        case 1: gao_scan_parties_range_kernel<FrP, 1><<<grid1, blk, 0, st>>>(c, a.ld, sh, rd, k, rho, a.listed, status, errpos, wk); break;
        case 2: gao_scan_parties_range_kernel<FrP, 2><<<grid1, blk, 0, st>>>(c, a.ld, sh, rd, k, rho, a.listed, status, errpos, wk); break;
        case 4: gao_scan_parties_range_kernel<FrP, 4><<<grid1, blk, 0, st>>>(c, a.ld, sh, rd, k, rho, a.listed, status, errpos, wk); break;
        default: gao_scan_parties_range_kernel<FrP, 8><<<grid1, blk, 0, st>>>(c, a.ld, sh, rd, k, rho, a.listed, status, errpos, wk); break;
      }
      const size_t gpb_r = GAO_THREADS / n;
      const dim3 grid_r((unsigned)std::min<size_t>((nchunks + gpb_r - 1) / gpb_r, GAO_STAGE2_GRID));
      gao_repair_parties_range_kernel<FrP><<<grid_r, blk, 0, st>>>(c, tab, inv->v, n, l, sh, rd, k, status, errpos, wk);
      GAO_HIP(hipGetLastError());
      return ZK_OK;
    }
  }
  if constexpr (REPAIR) switch (l) {
    case 1: gao_scan_parties_kernel<FrP, 1><<<grid1, blk, 0, st>>>(c, a.ld, sh, nchunks, k, rho, a.listed, status, errpos, wk); break;
    case 2: gao_scan_parties_kernel<FrP, 2><<<grid1, blk, 0, st>>>(c, a.ld, sh, nchunks, k, rho, a.listed, status, errpos, wk); break;
    case 4: gao_scan_parties_kernel<FrP, 4><<<grid1, blk, 0, st>>>(c, a.ld, sh, nchunks, k, rho, a.listed, status, errpos, wk); break;
    default: gao_scan_parties_kernel<FrP, 8><<<grid1, blk, 0, st>>>(c, a.ld, sh, nchunks, k, rho, a.listed, status, errpos, wk); break;
  }
  else switch (l) {
    case 1: gao_stage1_parties_kernel<FrP, 1><<<grid1, blk, 0, st>>>(c, a.ld, tab, sh, nchunks, k, rho, sec, msg, status, errpos, wk); break;
    case 2: gao_stage1_parties_kernel<FrP, 2><<<grid1, blk, 0, st>>>(c, a.ld, tab, sh, nchunks, k, rho, sec, msg, status, errpos, wk); break;
    case 4: gao_stage1_parties_kernel<FrP, 4><<<grid1, blk, 0, st>>>(c, a.ld, tab, sh, nchunks, k, rho, sec, msg, status, errpos, wk); break;
    default: gao_stage1_parties_kernel<FrP, 8><<<grid1, blk, 0, st>>>(c, a.ld, tab, sh, nchunks, k, rho, sec, msg, status, errpos, wk); break;
  }
  const size_t gpb = GAO_THREADS / n;
  const dim3 grid2((unsigned)std::min<size_t>((nchunks + gpb - 1) / gpb, GAO_STAGE2_GRID));
  if constexpr (REPAIR) gao_repair_parties_kernel<FrP><<<grid2, blk, 0, st>>>(c, tab, inv->v, n, l, sh, nchunks, k, status, errpos, wk);
  else gao_stage2_parties_kernel<FrP><<<grid2, blk, 0, st>>>(c, tab, n, l, sh, nchunks, k, sec, msg, status, errpos, wk);
  GAO_HIP(hipGetLastError());
  return ZK_OK;
}
template <class FrP>
int gao_unpack_robust_parties_run(IEngine* e, DevBuf& wkbuf, int l, const void* shares, const uint32_t* parties, int np,
                                  size_t nchunks, int dimension, void* secrets, void* message, uint8_t* status,
                                  uint32_t* errpos, uint64_t* summary, hipStream_t st) {
  return gao_party_list_run<FrP, false>(e, wkbuf, l, shares, parties, np, nchunks, dimension, secrets, message, status, errpos,
                                        summary, st);
}
template <class FrP>
int gao_repair_parties_run(IEngine* e, DevBuf& wkbuf, int l, void* shares, const uint32_t* parties, int np, size_t nchunks,
                           int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) {
  return gao_party_list_run<FrP, true>(e, wkbuf, l, shares, parties, np, nchunks, dimension, nullptr, nullptr, status, errpos,
                                       summary, st);
}
// The range form of zk_pss_repair_parties (gao.hpp): the word's rg.cnt valid columns lie in rows rg.stride elements apart,
// column c is chunk rg.chunk(c) of a word of rg.len chunks -- status and errpos [rg.len] are written there.  The list,
// dimension and summary are gao_repair_parties_run's; with no valid column only the summary is cleared.
template <class FrP>
int gao_repair_range_run(IEngine* e, DevBuf& wkbuf, int l, void* shares, const uint32_t* parties, int np, const GaoRange& rg,
                         int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) {
  if (rg.cnt > rg.stride || rg.cnt > rg.len || rg.base >= (rg.len ? rg.len : 1) || rg.shift > rg.len ||
      rg.stride > 0xffffffffull)
    return e->fail(ZK_ERR_BAD_INPUT, "bad range: cnt <= stride < 2^32, cnt <= len, base < len, shift <= len");
  int rc = gao_party_list_run<FrP, true>(e, wkbuf, l, shares, parties, np, rg.cnt, dimension, nullptr, nullptr, status, errpos,
                                         summary, st, &rg);
  if (rc || rg.cnt) return rc;
  if (summary) GAO_HIP(hipMemsetAsync(summary, 0, (size_t)(3 + 4 * l) * 8, st));
  return ZK_OK;
}
#undef GAO_HIP

}  // namespace zk
