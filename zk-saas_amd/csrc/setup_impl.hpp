// Kernels and host driver of zk_groth16_setup_scalars (setup.hpp says what they compute).  Included by setup_<curve>.hip only.
#pragma once
#include <algorithm>

#include "engine.hpp"
#include "ntt.hpp"
#include "setup.hpp"

namespace zk {

// elements per lane of quotient_kernel (a tunable of the kernel: one inversion costs about 35 products, an element 7 to 9)
constexpr uint32_t SETUP_RUN = 16;
// A column longer than this is summed by workgroups (setup_gather_heavy_kernel), a shorter one by one lane: the width of a
// wave -- a shorter column cannot give every lane of even one wave a term of a strided sum, and with one lane per column a
// wave lasts as long as its longest column, which this bounds at 64 multiply-adds.  Reasoned, not swept.
constexpr uint32_t SETUP_HEAVY_MIN = 64;
constexpr uint32_t SETUP_HEAVY_SPLIT = 4;       // workgroups per long column
constexpr uint32_t SETUP_HEAVY_GRID = 256;      // workgroup rows of the long-column kernel (they stride over the list)
constexpr uint32_t SETUP_SCAN_PER = 8;          // elements per thread of the scan tiles (256 threads)
constexpr uint32_t SETUP_SCAN_TILE = 256 * SETUP_SCAN_PER;

template <class F, class Term>
__global__ __launch_bounds__(256) void quotient_kernel(Term t, size_t len, uint32_t run, F* __restrict__ out) {
  size_t begin = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * run;
  if (begin >= len) return;
  size_t count = len - begin < run ? len - begin : run;
  quotient_run<F, Term>(t, begin, count, out);
}

// ---------------------------------------------------------------- (b) transposed sparse product
// The three matrices of one call (blockIdx.y picks one).  cnt / off: [nv + 1] per matrix; pairs: (row, nonzero) in column
// order, pair_base[k] = first pair of matrix k.
struct SetupMats {
  const uint32_t* row_ptr[3];
  const uint32_t* col[3];
  const void* val[3];
  uint32_t nnz[3];
  size_t pair_base[3];
};

// column histogram; a wire index >= nv is counted in *bad and takes no further part
static __global__ __launch_bounds__(256) void setup_hist_kernel(SetupMats M, uint32_t nv, uint32_t* __restrict__ cnt,
                                                         uint32_t* __restrict__ bad) {
  const int k = blockIdx.y;
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= M.nnz[k]) return;
  uint32_t c = M.col[k][e];
  if (c >= nv) {
    atomicAdd(bad, 1u);
    return;
  }
  atomicAdd(cnt + (size_t)k * (nv + 1) + c, 1u);
}

// exclusive scan of cnt[k][0 .. len) -> off[k][0 .. len), len = nv + 1 (cnt[k][nv] = 0, so off[k][nv] is the total), in three
// launches: tile sums, a scan of the tile sums by one workgroup per matrix, the tiles again with their offsets
__device__ __forceinline__ uint32_t block_scan_excl_256(uint32_t v, uint32_t* sh, uint32_t* total) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    uint32_t x = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  uint32_t incl = sh[t];
  *total = sh[255];
  __syncthreads();
  return incl - v;
}
static __global__ __launch_bounds__(256) void setup_scan_sums_kernel(const uint32_t* __restrict__ cnt, uint32_t len, uint32_t ntiles,
                                                              uint32_t* __restrict__ part) {
  __shared__ uint32_t sh[256];
  const int k = blockIdx.y;
  const uint32_t* c = cnt + (size_t)k * len;
  size_t base = (size_t)blockIdx.x * SETUP_SCAN_TILE + (size_t)threadIdx.x * SETUP_SCAN_PER;
  uint32_t s = 0;
  for (uint32_t j = 0; j < SETUP_SCAN_PER; j++)
    if (base + j < len) s += c[base + j];
  uint32_t total;
  (void)block_scan_excl_256(s, sh, &total);
  if (threadIdx.x == 0) part[(size_t)k * ntiles + blockIdx.x] = total;
}
static __global__ __launch_bounds__(256) void setup_scan_parts_kernel(uint32_t* __restrict__ part, uint32_t ntiles) {
  __shared__ uint32_t sh[256];
  uint32_t* p = part + (size_t)blockIdx.x * ntiles;
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < ntiles; b0 += 256) {           // (uniform trip count: every thread meets every barrier)
    uint32_t i = b0 + threadIdx.x;
    uint32_t v = i < ntiles ? p[i] : 0, total;
    uint32_t ex = block_scan_excl_256(v, sh, &total);
    if (i < ntiles) p[i] = carry + ex;
    carry += total;
  }
}
static __global__ __launch_bounds__(256) void setup_scan_apply_kernel(const uint32_t* __restrict__ cnt, uint32_t len, uint32_t ntiles,
                                                               const uint32_t* __restrict__ part, uint32_t* __restrict__ off) {
  __shared__ uint32_t sh[256];
  const int k = blockIdx.y;
  const uint32_t* c = cnt + (size_t)k * len;
  uint32_t* o = off + (size_t)k * len;
  size_t base = (size_t)blockIdx.x * SETUP_SCAN_TILE + (size_t)threadIdx.x * SETUP_SCAN_PER;
  uint32_t v[SETUP_SCAN_PER], s = 0;
#pragma unroll
  for (uint32_t j = 0; j < SETUP_SCAN_PER; j++) {
    v[j] = base + j < len ? c[base + j] : 0;
    s += v[j];
  }
  uint32_t total;
  uint32_t run = block_scan_excl_256(s, sh, &total) + part[(size_t)k * ntiles + blockIdx.x];
#pragma unroll
  for (uint32_t j = 0; j < SETUP_SCAN_PER; j++) {
    if (base + j < len) o[base + j] = run;
    run += v[j];
  }
}

// the row of nonzero e: the last r with row_ptr[r] <= e (empty rows repeat a value; the last of them is the one that holds e)
__device__ __forceinline__ uint32_t setup_row_of(const uint32_t* __restrict__ row_ptr, uint32_t nc, uint32_t e) {
  uint32_t lo = 0, hi = nc;                     // invariant: row_ptr[lo] <= e < row_ptr[hi]
  while (hi - lo > 1) {
    uint32_t mid = lo + (hi - lo) / 2;
    if (row_ptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}
// (row, nonzero) pairs into column order.  cnt counts down to zero: the slots of a column are handed out in arrival order,
// which the sums of the gather do not depend on (field addition is exact and commutative).
static __global__ __launch_bounds__(256) void setup_scatter_kernel(SetupMats M, uint32_t nv, uint32_t nc, uint32_t* __restrict__ cnt,
                                                            const uint32_t* __restrict__ off, uint2* __restrict__ pairs) {
  const int k = blockIdx.y;
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= M.nnz[k]) return;
  uint32_t c = M.col[k][e];
  if (c >= nv) return;
  uint32_t slot = atomicSub(cnt + (size_t)k * (nv + 1) + c, 1u) - 1;
  uint32_t pos = off[(size_t)k * (nv + 1) + c] + slot;
  if (pos >= M.nnz[k]) return;                  // (cannot happen: histogram and scatter see the same columns)
  pairs[M.pair_base[k] + pos] = make_uint2(setup_row_of(M.row_ptr[k], nc, (uint32_t)e), (uint32_t)e);
}

// One lane per column: a column of at most SETUP_HEAVY_MIN pairs is summed here, a longer one is entered into the list of
// long columns (matrix * nv + column; the list's order is arrival order and shows in no output).
template <class F>
__global__ __launch_bounds__(256) void setup_gather_kernel(SetupMats M, uint32_t nv, const uint32_t* __restrict__ off,
                                                           const uint2* __restrict__ pairs, const F* __restrict__ u,
                                                           F* __restrict__ acc, uint32_t* __restrict__ nheavy,
                                                           uint64_t* __restrict__ heavy, uint32_t heavy_cap) {
  const int k = blockIdx.y;
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nv) return;
  const uint32_t* o = off + (size_t)k * (nv + 1);
  uint32_t b = o[j], e = o[j + 1];
  if (e - b > SETUP_HEAVY_MIN) {
    uint32_t s = atomicAdd(nheavy, 1u);
    if (s < heavy_cap) heavy[s] = (uint64_t)k * nv + j;
    return;
  }
  const uint2* p = pairs + M.pair_base[k];
  const F* val = (const F*)M.val[k];
  F s = F::zero();
  for (uint32_t q = b; q < e; q++) {
    uint2 rk = p[q];
    s = s + load_elem(u + rk.x) * load_elem(val + rk.y);
  }
  store_elem(acc + (size_t)k * nv + j, s);
}

// Long columns: workgroup (x, y) takes the list entries x, x + gridDim.x, ... and of each the pairs y * 256 + tid, stepping
// by 256 * SETUP_HEAVY_SPLIT; its 256 partial sums are folded through LDS (limb-major, so that a wave's lanes read
// consecutive banks) and the workgroup's sum goes to part[entry][y].
template <class F>
__global__ __launch_bounds__(256) void setup_gather_heavy_kernel(SetupMats M, uint32_t nv, const uint32_t* __restrict__ off,
                                                                 const uint2* __restrict__ pairs, const F* __restrict__ u,
                                                                 const uint32_t* __restrict__ nheavy,
                                                                 const uint64_t* __restrict__ heavy, uint32_t heavy_cap,
                                                                 F* __restrict__ part) {
  __shared__ uint32_t sh[F::N][256];
  const uint32_t t = threadIdx.x;
  uint32_t nh = *nheavy;
  if (nh > heavy_cap) nh = heavy_cap;
  for (uint32_t h = blockIdx.x; h < nh; h += gridDim.x) {    // (block-uniform: every thread meets every barrier)
    const uint64_t id = heavy[h];
    const int k = (int)(id / nv);
    const size_t j = (size_t)(id % nv);
    const uint32_t* o = off + (size_t)k * (nv + 1);
    const uint32_t b = o[j], e = o[j + 1];
    const uint2* p = pairs + M.pair_base[k];
    const F* val = (const F*)M.val[k];
    F s = F::zero();
    for (size_t q = (size_t)b + blockIdx.y * 256 + t; q < e; q += 256 * SETUP_HEAVY_SPLIT) {
      uint2 rk = p[q];
      s = s + load_elem(u + rk.x) * load_elem(val + rk.y);
    }
#pragma unroll
    for (int i = 0; i < F::N; i++) sh[i][t] = s.v[i];
    __syncthreads();
    for (uint32_t d = 128; d >= 1; d >>= 1) {
      if (t < d) {
        F x;
#pragma unroll
        for (int i = 0; i < F::N; i++) x.v[i] = sh[i][t + d];
        s = s + x;
#pragma unroll
        for (int i = 0; i < F::N; i++) sh[i][t] = s.v[i];
      }
      __syncthreads();
    }
    if (t == 0) store_elem(part + (size_t)h * SETUP_HEAVY_SPLIT + blockIdx.y, s);
  }
}
// one lane per long column: the workgroups' sums in their fixed order
template <class F>
__global__ __launch_bounds__(256) void setup_heavy_fold_kernel(uint32_t nv, const uint32_t* __restrict__ nheavy,
                                                               const uint64_t* __restrict__ heavy, uint32_t heavy_cap,
                                                               const F* __restrict__ part, F* __restrict__ acc) {
  uint32_t nh = *nheavy;
  if (nh > heavy_cap) nh = heavy_cap;
  for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < nh; h += (size_t)gridDim.x * blockDim.x) {
    F s = load_elem(part + h * SETUP_HEAVY_SPLIT);
    for (uint32_t y = 1; y < SETUP_HEAVY_SPLIT; y++) s = s + load_elem(part + h * SETUP_HEAVY_SPLIT + y);
    store_elem(acc + heavy[h], s);              // (the list holds matrix * nv + column, the index into acc)
  }
}

// ---------------------------------------------------------------- (c) combine
template <class F>
struct SetupCombine {
  F alpha, beta, gamma_inv, delta_inv;
  const F* u;       // Lagrange coefficients [m]
  const F* acc;     // [3][nv]: A^T u, B^T u, C^T u
  F *a, *b, *l, *h, *abc;                       // outputs (any may be null)
  uint32_t nv, nc, ni;
  size_t m, tail;
};
// lane j < nv: a_j (+ u_{nc+j} below ni), b_j, (beta a_j + alpha b_j + c_j) / gamma below ni, / delta from ni up;
// lane nv + t, t < tail: the zero elements behind a, b, l and h
template <class F>
__global__ __launch_bounds__(256) void setup_combine_kernel(SetupCombine<F> c) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= c.nv) {
    size_t t = j - c.nv;
    if (t >= c.tail) return;
    const F z = F::zero();
    if (c.a) store_elem(c.a + c.nv + t, z);
    if (c.b) store_elem(c.b + c.nv + t, z);
    if (c.l) store_elem(c.l + (c.nv - c.ni) + t, z);
    if (c.h) store_elem(c.h + c.m + t, z);
    return;
  }
  F a = load_elem(c.acc + j), b = load_elem(c.acc + (size_t)c.nv + j), cc = load_elem(c.acc + 2 * (size_t)c.nv + j);
  if (j < c.ni) a = a + load_elem(c.u + c.nc + j);
  if (c.a) store_elem(c.a + j, a);
  if (c.b) store_elem(c.b + j, b);
  F abc = c.beta * a + c.alpha * b + cc;
  if (j < c.ni) {
    if (c.abc) store_elem(c.abc + j, abc * c.gamma_inv);
  } else if (c.l) {
    store_elem(c.l + (j - c.ni), abc * c.delta_inv);
  }
}


// ---------------------------------------------------------------- host driver
template <class FrP>
static Fp<FrP> setup_root_of_unity(int log_size) {
  Fp<FrP> r = Fp<FrP>::from_limbs(FrP::TWO_ADIC_ROOT);
  for (int i = log_size; i < FrP::TWO_ADICITY; i++) r = r.sqr();
  return r;
}
#define SETUP_HIP(expr)                                  \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return e->hip_fail(_e, #expr); \
  } while (0)

// Working memory wk: u [m], the three products [3][nv], the column counts and offsets, the pairs in column order, the list
// of long columns and their workgroup sums.
template <class FrP>
int setup_scalars_run(IEngine* e, DevBuf& wk, const void* const mats[9], size_t nvars, size_t nc, size_t ni, int log_m,
                      const void* trapdoor, size_t tail, void* const out[5], hipStream_t st) {
  using Fr = Fp<FrP>;
  if (!trapdoor || !mats[0] || !mats[3] || !mats[6]) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
  if (log_m < 0 || log_m > 30 || log_m + 1 > FrP::TWO_ADICITY) return e->fail(ZK_ERR_BAD_INPUT, "bad domain size");
  const size_t m = (size_t)1 << log_m;
  if (nc + ni > m) return e->fail(ZK_ERR_BAD_INPUT, "domain smaller than num_constraints + num_inputs");
  if (ni < 1 || ni > nvars || nvars >= ((size_t)1 << 32) - 1 || nc >= ((size_t)1 << 32))
    return e->fail(ZK_ERR_BAD_INPUT, "bad R1CS dimensions");
  // ---- the trapdoor, on the host, before any launch
  const uint32_t* td = (const uint32_t*)trapdoor;
  const Fr alpha = Fr::from_limbs(td), beta = Fr::from_limbs(td + Fr::N), gamma = Fr::from_limbs(td + 2 * Fr::N),
           delta = Fr::from_limbs(td + 3 * Fr::N), tau = Fr::from_limbs(td + 4 * Fr::N);
  if (gamma.is_zero()) return e->fail(ZK_ERR_BAD_INPUT, "degenerate trapdoor: gamma is zero");
  if (delta.is_zero()) return e->fail(ZK_ERR_BAD_INPUT, "degenerate trapdoor: delta is zero");
  if (tau.is_zero()) return e->fail(ZK_ERR_BAD_INPUT, "degenerate trapdoor: tau is zero");
  Fr tau_m = tau;
  for (int i = 0; i < log_m; i++) tau_m = tau_m.sqr();
  const Fr tau_n = tau_m.sqr();
  if (tau_n == Fr::one())
    return e->fail(ZK_ERR_BAD_INPUT, "degenerate trapdoor: tau lies in the evaluation domain of size 2m (tau^(2m) = 1)");
  const Fr w = setup_root_of_unity<FrP>(log_m), w2 = setup_root_of_unity<FrP>(log_m + 1), w2_inv = w2.inverse();
  LagrangeTerm<Fr> lt{tau, (tau_m - Fr::one()) * Fr::from_u64(m).inverse(), w, w.inverse()};
  HTerm<Fr> ht{tau, tau_n, (delta * Fr::from_u64(2 * m)).inverse(), w2_inv.sqr(), w, w2_inv};
  // ---- sizes: the nonzero counts are the last row pointers
  SetupMats M{};
  uint32_t nnz[3] = {0, 0, 0};
  for (int k = 0; k < 3; k++) {
    M.row_ptr[k] = (const uint32_t*)mats[3 * k];
    M.col[k] = (const uint32_t*)mats[3 * k + 1];
    M.val[k] = mats[3 * k + 2];
    SETUP_HIP(hipMemcpyAsync(&nnz[k], M.row_ptr[k] + nc, 4, hipMemcpyDeviceToHost, st));
  }
  SETUP_HIP(hipStreamSynchronize(st));
  size_t total = 0;
  uint32_t nnz_max = 0;
  for (int k = 0; k < 3; k++) {
    if (nnz[k] && (!M.col[k] || !M.val[k])) return e->fail(ZK_ERR_BAD_INPUT, "null pointer");
    M.nnz[k] = nnz[k];
    M.pair_base[k] = total;
    total += nnz[k];
    nnz_max = std::max(nnz_max, nnz[k]);
  }
  const uint32_t nv = (uint32_t)nvars, len = nv + 1, ntiles = (len + SETUP_SCAN_TILE - 1) / SETUP_SCAN_TILE;
  const uint32_t heavy_cap = (uint32_t)(total / (SETUP_HEAVY_MIN + 1)) + 1;
  // ---- working memory (every part a multiple of 32 bytes)
  auto r32 = [](size_t b) { return (b + 31) / 32 * 32; };
  const size_t b_u = m * sizeof(Fr), b_acc = 3 * (size_t)nv * sizeof(Fr), b_cnt = r32(3 * (size_t)len * 4 + 8),
               b_off = r32(3 * (size_t)len * 4), b_part = r32(3 * (size_t)ntiles * 4), b_pairs = r32(total * 8),
               b_heavy = r32((size_t)heavy_cap * 8), b_hpart = (size_t)heavy_cap * SETUP_HEAVY_SPLIT * sizeof(Fr);
  SETUP_HIP(wk.ensure(b_u + b_acc + b_cnt + b_off + b_part + b_pairs + b_heavy + b_hpart));
  char* p = (char*)wk.p;
  Fr* u = (Fr*)p;
  Fr* acc = (Fr*)(p += b_u);
  uint32_t* cnt = (uint32_t*)(p += b_acc);
  uint32_t* bad = cnt + 3 * (size_t)len;          // [0] wire indices out of range, [1] long columns
  uint32_t* off = (uint32_t*)(p += b_cnt);
  uint32_t* part = (uint32_t*)(p += b_off);
  uint2* pairs = (uint2*)(p += b_part);
  uint64_t* heavy = (uint64_t*)(p += b_pairs);
  Fr* hpart = (Fr*)(p += b_heavy);
  const dim3 blk(256);
  auto grid = [](size_t work, unsigned y = 1) { return dim3((unsigned)((work + 255) / 256), y); };
  // ---- (a) Lagrange coefficients and h_query
  quotient_kernel<Fr, LagrangeTerm<Fr>><<<grid((m + SETUP_RUN - 1) / SETUP_RUN), blk, 0, st>>>(lt, m, SETUP_RUN, u);
  if (out[3])
    quotient_kernel<Fr, HTerm<Fr>><<<grid((m + SETUP_RUN - 1) / SETUP_RUN), blk, 0, st>>>(ht, m, SETUP_RUN, (Fr*)out[3]);
  // ---- (b) column order, then the three products
  SETUP_HIP(hipMemsetAsync(cnt, 0, b_cnt, st));
  if (nnz_max) setup_hist_kernel<<<grid(nnz_max, 3), blk, 0, st>>>(M, nv, cnt, bad);
  setup_scan_sums_kernel<<<dim3(ntiles, 3), blk, 0, st>>>(cnt, len, ntiles, part);
  setup_scan_parts_kernel<<<dim3(3), blk, 0, st>>>(part, ntiles);
  setup_scan_apply_kernel<<<dim3(ntiles, 3), blk, 0, st>>>(cnt, len, ntiles, part, off);
  if (nnz_max) setup_scatter_kernel<<<grid(nnz_max, 3), blk, 0, st>>>(M, nv, (uint32_t)nc, cnt, off, pairs);
  setup_gather_kernel<Fr><<<grid(nv, 3), blk, 0, st>>>(M, nv, off, pairs, u, acc, bad + 1, heavy, heavy_cap);
  setup_gather_heavy_kernel<Fr><<<dim3(std::min(heavy_cap, SETUP_HEAVY_GRID), SETUP_HEAVY_SPLIT), blk, 0, st>>>(
      M, nv, off, pairs, u, bad + 1, heavy, heavy_cap, hpart);
  setup_heavy_fold_kernel<Fr><<<grid(std::min<size_t>(heavy_cap, 1 << 16)), blk, 0, st>>>(nv, bad + 1, heavy, heavy_cap, hpart,
                                                                                        acc);
  // ---- (c) combine and the zero tails
  SetupCombine<Fr> cb{alpha, beta, gamma.inverse(), delta.inverse(), u, acc, (Fr*)out[0], (Fr*)out[1], (Fr*)out[2],
                      (Fr*)out[3], (Fr*)out[4], nv, (uint32_t)nc, (uint32_t)ni, m, tail};
  setup_combine_kernel<Fr><<<grid((size_t)nv + tail), blk, 0, st>>>(cb);
  SETUP_HIP(hipGetLastError());
  uint32_t nbad = 0;
  SETUP_HIP(hipMemcpyAsync(&nbad, bad, 4, hipMemcpyDeviceToHost, st));
  SETUP_HIP(hipStreamSynchronize(st));
  if (nbad) return e->fail(ZK_ERR_GENERIC, "R1CS wire index out of range");
  return ZK_OK;
}
#undef SETUP_HIP

}  // namespace zk
