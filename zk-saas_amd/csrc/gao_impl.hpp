// Kernels and host driver of zk_pss_unpack_robust (gao.hpp says what they compute).  Included by gao_<curve>.hip only.
//   stage 1  one lane per chunk (two at l = 8): the n shares are loaded once, transformed in registers, coefficients k .. n - 1 tested; a
//            clean chunk gets its secrets (and message) and status 0, a dirty one is appended to a compact list
//   stage 2  one group of n lanes per listed chunk: Gao's decoder (gao_chunk) over the wave's cross-lane builtins.  Launched
//            unconditionally with a grid derived from nchunks; it reads the count from device memory, strides over the list and
//            leaves at once when the count is zero -- so the call never synchronises with the host.
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
template <class P, int L>
__global__ __launch_bounds__(GAO_THREADS) void gao_stage1_kernel(const GaoConsts<Fp<P>> c, const Fp<P>* __restrict__ shares,
                                                                size_t nchunks, int k, Fp<P>* __restrict__ secrets,
                                                                Fp<P>* __restrict__ message, uint8_t* __restrict__ status,
                                                                uint32_t* __restrict__ errpos, GaoWork wk) {
  using F = Fp<P>;
  constexpr int N = 4 * L, SP = gao_split(L), M = N / SP;
  __shared__ uint32_t wg_dirty, wg_base;
  if (threadIdx.x == 0) wg_dirty = 0;
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, j = t / SP;
  const int q = (int)(t % SP);
  const bool live = j < nchunks;         // (the SP lanes of a chunk are neighbours and agree)
  bool dirty = false;
  if (live) {
    F x[M];
    gao_load<M, SP>(c, q, [&](int p) { return load_elem(shares + (size_t)p * nchunks + j); }, x);
    gao_ifft<M, SP>(c, x);
    dirty = !gao_is_clean<M, SP>(x, k, q);
    if (SP == 2) dirty = __shfl_xor((int)dirty, 1, 64) || dirty;
    if (!dirty) {
      if (q == 0) {
        status[j] = 0;
        if (errpos) errpos[j] = 0;
      }
      if (message)
        gao_clean_message<M, SP>(c, x, k, q, [&](int i, const F& v) { store_elem(message + (size_t)i * nchunks + j, v); });
      if (secrets)
        gao_clean_secrets<M, SP>(c, x, k, q, [&](int i, const F& v) {
          F sum = v;
          if (SP == 2) {           // the two lanes of the chunk are both here: add their parts
            F o;
#pragma unroll
            for (int w = 0; w < F::N; w++) o.v[w] = (uint32_t)__shfl_xor((int)v.v[w], 1, 64);
            sum = v + o;
          }
          if (q == 0) store_elem(secrets + j * L + i, sum);
        });
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
  if (dirty) wk.list[wg_base + wave_off + rank] = (uint32_t)j;
}

// ---------------------------------------------------------------- stage 2
template <class P>
__global__ __launch_bounds__(GAO_THREADS) void gao_stage2_kernel(const GaoConsts<Fp<P>> c, int n, int l,
                                                                const Fp<P>* __restrict__ shares, size_t nchunks, int k,
                                                                Fp<P>* __restrict__ secrets, Fp<P>* __restrict__ message,
                                                                uint8_t* __restrict__ status, uint32_t* __restrict__ errpos,
                                                                GaoWork wk) {
  using F = Fp<P>;
  const uint32_t cnt = *wk.count;
  const uint32_t gpb = GAO_THREADS / n, stride = gridDim.x * gpb;
  if (blockIdx.x * gpb >= cnt) return;
  const int p = threadIdx.x % n;
  const GaoDevGroup g{n, p, (int)(threadIdx.x & 63) / n * n};
  // this lane's points: w^p, w^-p and (lanes < l) g w_2l^p
  const F xp = gao_lane_pow<F, 5>(c.wpow2, p), xinv = gao_lane_pow<F, 5>(c.wipow2, p);
  const F sp = c.g * gao_lane_pow<F, 3>(c.spow2, p & 7);
  uint32_t n_fixed = 0, n_status1 = 0, n_status2 = 0;       // this lane's part of the summary, added once at the end
  for (uint32_t first = blockIdx.x * gpb; first < cnt; first += stride) {       // (uniform over the workgroup)
    const uint32_t gi = first + threadIdx.x / n;
    const bool live = gi < cnt;
    const size_t j = live ? wk.list[gi] : 0;
    const F y = live ? load_elem(shares + (size_t)p * nchunks + j) : F::zero();
    const GaoResult<F, GaoDevGroup> r = gao_chunk<F, GaoDevGroup>(g, c, n, k, live, y, xp, xinv, sp);
    if (!live) continue;
    if (message && p < k) store_elem(message + (size_t)p * nchunks + j, r.h);
    if (secrets && p < l) store_elem(secrets + j * l + p, r.sec);
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
#define GAO_HIP(expr)                                    \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return e->hip_fail(_e, #expr); \
  } while (0)

template <class FrP>
int gao_unpack_robust_run(IEngine* e, DevBuf& wkbuf, int l, const void* shares, size_t nchunks, int dimension, void* secrets,
                          void* message, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) {
  using Fr = Fp<FrP>;
  const int n = 4 * l;
  if (dimension < 1 || dimension > n - 1) return e->fail(ZK_ERR_BAD_INPUT, "dimension must lie in 1 .. n - 1");
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
  const Fr* sh = (const Fr*)shares;
  Fr* sec = (Fr*)secrets;
  Fr* msg = (Fr*)message;
  switch (l) {
    case 1: gao_stage1_kernel<FrP, 1><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, sec, msg, status, errpos, wk); break;
    case 2: gao_stage1_kernel<FrP, 2><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, sec, msg, status, errpos, wk); break;
    case 4: gao_stage1_kernel<FrP, 4><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, sec, msg, status, errpos, wk); break;
    case 8: gao_stage1_kernel<FrP, 8><<<grid1, blk, 0, st>>>(c, sh, nchunks, dimension, sec, msg, status, errpos, wk); break;
    default: return e->fail(ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8");
  }
  const size_t gpb = GAO_THREADS / n;
  const dim3 grid2((unsigned)std::min<size_t>((nchunks + gpb - 1) / gpb, GAO_STAGE2_GRID));
  gao_stage2_kernel<FrP><<<grid2, blk, 0, st>>>(c, n, l, sh, nchunks, dimension, sec, msg, status, errpos, wk);
  GAO_HIP(hipGetLastError());
  return ZK_OK;
}
#undef GAO_HIP

}  // namespace zk
