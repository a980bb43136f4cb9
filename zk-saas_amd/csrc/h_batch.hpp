// The h chain (engine_h.inc.hpp h_chain): the layout of its work buffer, where the report rows of a checked batch lie while
// the chain runs, and the three launches the checked chain adds to the unchecked one's.
//   - h_layout: the byte offsets of the regions of the work buffer, for every form of the chain.  Plain integers only.
//   - staging_row: the repair of a round indexes status and errpos by item * nchunks + chunk (gao_impl.hpp), so the rows of
//     one ROUND are contiguous; the caller's report is proof-major, [nb][7].  The three repairs write a round-major staging
//     report and ONE gather launch at the end of the chain moves every row to its place.  Plain integers only: this part
//     compiles for the host alone (tests/native/h_batch_rows_host_test.cpp).
//   - h_words_batch_kernel: the king words of a whole round in place, one launch for up to 48 items
//   - h_mulsub_batch_kernel: the deg_red words a*b - c (+ in_mask) of all proofs, one launch
//   - h_report_gather_kernel: staging rows -> the proof-major report
// The pointer tables travel BY VALUE in the kernel arguments, as KingBatch does (pss.hpp); blockIdx.y selects the item, so its
// pointer is uniform per workgroup.  No LDS, no scratch, one grid-stride loop each.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ZK_HB_HD __host__ __device__ __forceinline__
#else
#define ZK_HB_HD inline
#endif

namespace zk {

constexpr int H_BATCH_MAX = 16;                    // DEGRED_BATCH, MAX_PROOF_BATCH: the proofs of one batch
constexpr int H_BATCH_ITEMS = 3 * H_BATCH_MAX;     // KING_BATCH, GAO_BATCH_MAX: the items of one round
constexpr int H_REPORT_ROWS = 7;                   // the king words of one proof (zk_circom_h_checked)

// the staging row of item k (0..6) of proof b in a batch of nb: round 1 (k < 3) holds rows [0, 3 nb), item 3 b + k of its
// repair; round 2 (k < 6) rows [3 nb, 6 nb); the deg_red round rows [6 nb, 7 nb), item b
ZK_HB_HD uint32_t staging_row(uint32_t nb, uint32_t b, uint32_t k) {
  return k < 3 ? 3 * b + k : k < 6 ? 3 * nb + 3 * b + (k - 3) : 6 * nb + b;
}
// the first staging row of a round (0, 1: the d_ifft / d_fft words; 2: the deg_red words) and its number of items
ZK_HB_HD uint32_t staging_round_first(uint32_t nb, uint32_t round) { return round < 2 ? 3 * nb * round : 6 * nb; }
ZK_HB_HD uint32_t staging_round_items(uint32_t nb, uint32_t round) { return round < 2 ? 3 * nb : nb; }

// The work buffer of an h chain (h_chain's hwork) in byte offsets, a region's start a multiple of 32: W0 at 0 and W1, 3 nb vectors
// [n][nchunks] of `elem` bytes an element each; the checked chain: the repair's working memory, gao_bytes =
// gao_layout<Fr>(n, 3 nb, nchunks, listed).bytes of them (0: the unchecked chain); a checked batch (nb > 1): the round-major
// staging status, errpos and summary rows.  A region that the form does not have is empty and lies at the end.
struct HLayout {
  size_t w1, gao, status, errpos, summary, bytes;
};
ZK_HB_HD HLayout h_layout(size_t n, size_t nb, size_t nchunks, size_t elem, size_t gao_bytes, bool errpos, bool summary) {
  const size_t rows = gao_bytes && nb > 1 ? H_REPORT_ROWS * nb : 0;
  HLayout w;
  w.w1 = 3 * n * nchunks * nb * elem;
  w.gao = 2 * w.w1;
  w.status = w.bytes = w.gao + gao_bytes;
  if (rows) w.status = (w.status + 31) / 32 * 32;
  w.errpos = w.status + (rows * nchunks + 31) / 32 * 32;
  w.summary = w.errpos + ((errpos ? rows * nchunks * 4 : 0) + 31) / 32 * 32;
  if (rows) w.bytes = w.summary + (summary ? rows * (3 + n) * 8 : 0);
  return w;
}

}  // namespace zk

#if defined(__HIPCC__)
#include "ntt.hpp"

namespace zk {

template <class F>
struct HWordMasks {
  const F* mask[H_BATCH_ITEMS];
};
// item y = blockIdx.y is the vector [len] at w + y * stride: W * (scale ? k : 1) + mask[y]; an item without a mask keeps its
// bytes (its workgroups leave at once).  scale: the inverse round, k = 1 / m.
template <class F>
__global__ __launch_bounds__(256) void h_words_batch_kernel(F* __restrict__ w, size_t stride, HWordMasks<F> hm, int scale, F k,
                                                            size_t len) {
  const F* __restrict__ mask = hm.mask[blockIdx.y];
  if (!mask) return;
  __builtin_amdgcn_s_setprio(3);   // on the circom_h chain (see vec_mul_sub_kernel)
  F* __restrict__ x = w + blockIdx.y * stride;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += step) {
    F v = load_elem(x + i);
    if (scale) v = v * k;
    store_elem(x + i, v + load_elem(mask + i));
  }
}

template <class F>
struct HProdMasks {
  const F* mask[H_BATCH_MAX];
};
// proof y = blockIdx.y: out + y * out_step = a * b - c (+ mask[y]), a, b, c the vectors [len] at in + y * in_step + {0, 1, 2}
// * len (the second king's output of a batch).  out does not alias in.
template <class F>
__global__ __launch_bounds__(256) void h_mulsub_batch_kernel(F* __restrict__ out, size_t out_step, const F* __restrict__ in,
                                                             size_t in_step, HProdMasks<F> hm, size_t len) {
  __builtin_amdgcn_s_setprio(3);
  const F* __restrict__ mask = hm.mask[blockIdx.y];
  const F* __restrict__ a = in + blockIdx.y * in_step;
  const F* __restrict__ b = a + len;
  const F* __restrict__ c = b + len;
  F* __restrict__ o = out + blockIdx.y * out_step;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += step) {
    F v = load_elem(a + i) * load_elem(b + i) - load_elem(c + i);
    if (mask) v = v + load_elem(mask + i);
    store_elem(o + i, v);
  }
}

// the report of a batch from its round-major staging rows: blockIdx.y = 7 b + k is a row of the proof-major report, read at
// staging_row(nb, b, k).  status [rows][nchunks] bytes, errpos [rows][nchunks] words (both null or both set), summary
// [rows][sum_words] 64-bit counters (both null or both set).
static __global__ __launch_bounds__(256) void h_report_gather_kernel(uint32_t nb, uint32_t nchunks, uint32_t sum_words,
                                                                     const uint8_t* __restrict__ st_in,
                                                                     const uint32_t* __restrict__ ep_in,
                                                                     const uint64_t* __restrict__ sm_in,
                                                                     uint8_t* __restrict__ st_out, uint32_t* __restrict__ ep_out,
                                                                     uint64_t* __restrict__ sm_out) {
  const uint32_t row = blockIdx.y;
  const size_t src = staging_row(nb, row / H_REPORT_ROWS, row % H_REPORT_ROWS);
  const uint32_t step = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t i = t0; i < nchunks; i += step) {
    st_out[(size_t)row * nchunks + i] = st_in[src * nchunks + i];
    if (ep_out) ep_out[(size_t)row * nchunks + i] = ep_in[src * nchunks + i];
  }
  if (sm_out && t0 < sum_words) sm_out[(size_t)row * sum_words + t0] = sm_in[src * sum_words + t0];
}

// launch shape of the three: 256 threads, grid.y = items, grid.x covers the vector at one element per thread, capped so that
// the grid stays near 2048 workgroups (rows.hpp); the rest is walked by the grid-stride loop
inline dim3 h_batch_grid(size_t len, int items) {
  size_t gx = (len + 255) / 256, cap = 2048 / (size_t)items;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  return dim3((unsigned)gx, (unsigned)items);
}

}  // namespace zk
#endif
