// Kernels and host driver of zk_pss_unpack_points_robust and zk_pss_repair_points (gao_points.hpp says what they compute).
// Included by gao_points_<curve>.hip only.  With LIST the same two stages serve a party list (zk_pss_unpack_points_robust_parties,
// zk_pss_repair_points_parties): the shares are the compact [np][nchunks], the syndrome rows and the matrix come from the
// list's table (GaoPtList) and stage 2 looks a named party's row up in it; the LIST = false kernels read none of it.
//   stage 1  the scan: a workgroup takes 64 chunks, one per lane of a wave; its four waves share out the rows -- the n - k
//            syndromes, then (with an output) the l secrets of the plain unpack -- so all lanes of a wave walk one coefficient
//            row and every bit test of the double-and-add is uniform.  A syndrome is tested as it stands (ZZ == 0) and stored
//            in affine form for stage 2; a chunk whose syndromes are all the identity gets status 0, the others go onto a
//            compact list.  The secrets are written for every chunk: those of a dirty chunk are what stage 2 corrects.
//   stage 2  one group of n lanes per listed chunk (gao_points_chunk over the wave's ballot).  Launched unconditionally with a
//            grid derived from nchunks; it reads the count from device memory and strides over the list, so the call never
//            synchronises with the host.
// Stage 2 takes the syndromes from working memory rather than recomputing them: a recomputation in a lane group would walk
// n - k different coefficient rows in one wave, every bit test divergent, for rows stage 1 has just finished.
#pragma once
#include <algorithm>

#include "gao_impl.hpp"
#include "gao_points.hpp"
#include "ntt.hpp"

namespace zk {

constexpr int GAO_PT_CHUNKS = 64;        // chunks per workgroup of the scan

template <class Fld>
struct GaoPtWork {
  uint32_t* count;                       // number of dirty chunks
  unsigned long long* summary;           // [3 + n]: clean, corrected, failed, corrections per party
  uint32_t* list;                        // the dirty chunks
  Affine<Fld>* syn;                      // [n - k][nchunks]: the syndromes
};

// ---------------------------------------------------------------- stage 1
template <class FrP, class Fld, bool LIST>
__global__ __launch_bounds__(GAO_THREADS) void gao_points_scan_kernel(const GaoPtTable<Fp<FrP>>* __restrict__ tab,
                                                                     const Fp<FrP>* __restrict__ umat, int n, int l, int k,
                                                                     const Affine<Fld>* shares, size_t nchunks,
                                                                     Affine<Fld>* out, uint8_t* __restrict__ status,
                                                                     uint32_t* __restrict__ errpos, GaoPtWork<Fld> wk,
                                                                     GaoPtList<Fp<FrP>> lt) {
  __shared__ uint32_t dirty_lds[GAO_PT_CHUNKS];
  const uint32_t lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x < GAO_PT_CHUNKS) dirty_lds[threadIdx.x] = 0;
  __syncthreads();
  const size_t j = (size_t)blockIdx.x * GAO_PT_CHUNKS + lane;
  const bool live = j < nchunks;
  const int np = LIST ? lt.np : n;                                // the rows of `shares`, and a coefficient row's length
  const int nsyn = np - k, nrows = nsyn + (out ? l : 0);
  if (live)
    for (int r = wave; r < nrows; r += GAO_THREADS / 64) {       // (uniform over the wave)
      const bool is_syn = r < nsyn;
      const XYZZ<Fld> acc = gao_points_row<FrP, Fld>(
          np,
          [&](int p) {
            if constexpr (LIST) return is_syn ? lt.syn + (size_t)r * np + p : umat + (size_t)(r - nsyn) * np + p;
            else return is_syn ? gao_points_syn_coef(tab, n, k, r, p) : umat + (size_t)(r - nsyn) * n + p;
          },
          [&](int p) { return load_elem(shares + (size_t)p * nchunks + j); });
      if (is_syn) {
        if (!acc.is_identity()) dirty_lds[lane] = 1;
        store_elem(wk.syn + (size_t)r * nchunks + j, gao_pt_to_affine(acc));
      } else {
        store_elem(out + j * (size_t)l + (r - nsyn), gao_pt_to_affine(acc));
      }
    }
  __syncthreads();
  if (wave != 0) return;
  // the dirty chunks of the workgroup take consecutive places: one global atomic
  const bool dirty = live && dirty_lds[lane];
  if (live && !dirty) {
    status[j] = 0;
    if (errpos) errpos[j] = 0;
  }
  const uint64_t m = __ballot(dirty);
  const uint32_t nd = (uint32_t)__popcll(m), rank = (uint32_t)__popcll(m & (((uint64_t)1 << lane) - 1));
  uint32_t base = 0;
  if (lane == 0) {
    const size_t first = (size_t)blockIdx.x * GAO_PT_CHUNKS;
    const uint32_t in_wg = (uint32_t)(nchunks - first < GAO_PT_CHUNKS ? nchunks - first : GAO_PT_CHUNKS);
    if (nd) base = atomicAdd(wk.count, nd);
    if (in_wg > nd) atomicAdd(wk.summary, (unsigned long long)(in_wg - nd));
  }
  base = (uint32_t)__shfl((int)base, 0, 64);
  if (dirty) wk.list[base + rank] = (uint32_t)j;
}

// ---------------------------------------------------------------- stage 2
// REPAIR: `shares` is written: lane 0 stores Y_q - E over the share of the party errpos names.  Otherwise lane i < l stores
// secret i of the corrected word over what stage 1 wrote, or the identity for a failed chunk (out may be null: verdicts only).
template <class Fld, bool REPAIR>
using GaoPtSharesPtr = std::conditional_t<REPAIR, Affine<Fld>*, const Affine<Fld>*>;
template <class FrP, class Fld, bool REPAIR, bool LIST>
__global__ __launch_bounds__(GAO_THREADS) void gao_points_stage2_kernel(const GaoPtTable<Fp<FrP>>* __restrict__ tab,
                                                                       const Fp<FrP>* __restrict__ umat, int n, int l, int k,
                                                                       GaoPtSharesPtr<Fld, REPAIR> shares, size_t nchunks,
                                                                       Affine<Fld>* out, uint8_t* __restrict__ status,
                                                                       uint32_t* __restrict__ errpos, GaoPtWork<Fld> wk,
                                                                       GaoPtList<Fp<FrP>> lt) {
  using Fr = Fp<FrP>;
  const uint32_t cnt = *wk.count;
  const uint32_t gpb = GAO_THREADS / n, stride = gridDim.x * gpb;
  if (blockIdx.x * gpb >= cnt) return;
  const int p = threadIdx.x % n;
  const GaoDevGroup g{n, p, (int)(threadIdx.x & 63) / n * n};
  const int nfix = REPAIR ? 1 : (out ? l : 0);
  uint32_t n_fixed = 0, n_status1 = 0, n_status2 = 0;       // this lane's part of the summary, added once at the end
  for (uint32_t first = blockIdx.x * gpb; first < cnt; first += stride) {       // (uniform over the workgroup)
    const uint32_t gi = first + threadIdx.x / n;
    const bool live = gi < cnt;
    const size_t j = live ? wk.list[gi] : 0;
    const auto syn = [&](int i) { return load_elem(wk.syn + (size_t)i * nchunks + j); };
    const auto row = [&](int q) {                                   // party q's row of the shares and column of the matrix
      if constexpr (LIST) return (int)lt.row[q];
      else return q;
    };
    const auto base = [&](int q, int i) {
      if constexpr (REPAIR) return load_elem(shares + (size_t)row(q) * nchunks + j);
      else return load_elem(out + j * (size_t)l + i);
    };
    const auto ucoef = [&](int i, int q) {
      return REPAIR ? Fr::zero() : load_elem(umat + (size_t)i * (LIST ? lt.np : n) + row(q));
    };
    // gao_points_chunk or gao_points_chunk_parties, one call for both (a result chosen after the fact would be a select over
    // point aggregates)
    const GaoPtResult<Fld, GaoDevGroup> r = gao_points_chunk_on<FrP, Fld, GaoDevGroup, REPAIR>(
        g, tab, n, (LIST ? lt.np : n) - k, nfix, live, syn, base, ucoef,
        [&](int c) {
          if constexpr (LIST) return gao_points_listed(lt, c);
          else return true;
        },
        [&](int q) {
          if constexpr (LIST) return lt.fix[q];
          else return gao_points_err_scalar(tab, n, k, q);
        });
    if (!live) continue;
    if constexpr (REPAIR) {
      if (r.status == 1 && p == 0) store_elem(shares + (size_t)row(gao_top_bit(r.errpos)) * nchunks + j, r.val);
    } else {
      if (p < nfix) store_elem(out + j * (size_t)l + p, r.val);
    }
    if (p == 0) {
      status[j] = (uint8_t)r.status;
      if (errpos) errpos[j] = r.errpos;
      if (r.status == 1) n_status1++;
      else n_status2++;
    }
    n_fixed += (r.errpos >> p) & 1;
  }
  if (n_status1) atomicAdd(wk.summary + 1, (unsigned long long)n_status1);
  if (n_status2) atomicAdd(wk.summary + 2, (unsigned long long)n_status2);
  if (n_fixed) atomicAdd(wk.summary + 3 + p, (unsigned long long)n_fixed);
}

// ---------------------------------------------------------------- host driver
#define GAO_PT_HIP(expr)                                 \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return e->hip_fail(_e, #expr); \
  } while (0)

template <class FrP, class Fld, bool REPAIR>
int gao_points_run(IEngine* e, DevBuf& wkbuf, int l, std::conditional_t<REPAIR, void*, const void*> shares, size_t nchunks,
                   int dimension, const GaoPtTable<Fp<FrP>>* tab, const Fp<FrP>* umat, const GaoPtList<Fp<FrP>>* list, void* out,
                   uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) {
  using A = Affine<Fld>;
  const int n = 4 * l;
  if (l != 1 && l != 2 && l != 4 && l != 8) return e->fail(ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8");
  if (dimension < 1 || dimension > n - 1) return e->fail(ZK_ERR_BAD_INPUT, "dimension must lie in 1 .. n - 1");
  if (nchunks == 0) return ZK_OK;
  if (!shares || !status) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
  if (nchunks >= ((size_t)1 << 32)) return e->fail(ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks");
  if (list) umat = list->umat;
  if (!tab || (!REPAIR && out && !umat)) return e->fail(ZK_ERR_GENERIC, "decoder table or unpack matrix missing");
  const int np = list ? list->np : n;
  if (np <= dimension || np > n) return e->fail(ZK_ERR_GENERIC, "party list does not fit the dimension");
  const int nsyn = np - dimension;
  // the count, then the summary words from byte 32 on; the list; the syndromes
  constexpr size_t head = 320;
  static_assert(32 + (3 + GAO_MAX_N) * 8 <= head && head % 32 == 0, "layout");
  const size_t list_bytes = (nchunks * 4 + 31) / 32 * 32;
  GAO_PT_HIP(wkbuf.ensure(head + list_bytes + (size_t)nsyn * nchunks * sizeof(A)));
  GaoPtWork<Fld> wk;
  wk.count = (uint32_t*)wkbuf.p;
  wk.summary = summary ? (unsigned long long*)summary : (unsigned long long*)((char*)wkbuf.p + 32);
  wk.list = (uint32_t*)((char*)wkbuf.p + head);
  wk.syn = (A*)((char*)wkbuf.p + head + list_bytes);
  GAO_PT_HIP(hipMemsetAsync(wkbuf.p, 0, head, st));
  if (summary) GAO_PT_HIP(hipMemsetAsync(summary, 0, (size_t)(3 + n) * 8, st));
  const dim3 blk(GAO_THREADS);
  GaoPtSharesPtr<Fld, REPAIR> sh = (GaoPtSharesPtr<Fld, REPAIR>)shares;
  const dim3 grid1((unsigned)((nchunks + GAO_PT_CHUNKS - 1) / GAO_PT_CHUNKS));
  const size_t gpb = GAO_THREADS / n;
  const dim3 grid2((unsigned)std::min<size_t>((nchunks + gpb - 1) / gpb, GAO_STAGE2_GRID));
  if (list) {
    gao_points_scan_kernel<FrP, Fld, true><<<grid1, blk, 0, st>>>(tab, umat, n, l, dimension, sh, nchunks, (A*)out, status,
                                                                 errpos, wk, *list);
    gao_points_stage2_kernel<FrP, Fld, REPAIR, true><<<grid2, blk, 0, st>>>(tab, umat, n, l, dimension, sh, nchunks, (A*)out,
                                                                           status, errpos, wk, *list);
  } else {
    const GaoPtList<Fp<FrP>> none{};
    gao_points_scan_kernel<FrP, Fld, false><<<grid1, blk, 0, st>>>(tab, umat, n, l, dimension, sh, nchunks, (A*)out, status,
                                                                  errpos, wk, none);
    gao_points_stage2_kernel<FrP, Fld, REPAIR, false><<<grid2, blk, 0, st>>>(tab, umat, n, l, dimension, sh, nchunks, (A*)out,
                                                                            status, errpos, wk, none);
  }
  GAO_PT_HIP(hipGetLastError());
  return ZK_OK;
}
#undef GAO_PT_HIP

}  // namespace zk
