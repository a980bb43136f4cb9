// Robust unpack of packed POINT shares (zk_pss_unpack_points_robust, zk_pss_repair_points): the n = 4l shares Y_p of one chunk
// are a Reed-Solomon word "in the exponent" -- Y_p = y_p G for a word y no one sees.  Gao's decoder (gao.hpp) divides
// polynomials by their coefficients, and there is no division of group elements; what remains are fixed SCALAR combinations
// of the shares, which is enough to detect any error and to locate and correct one wrong share per chunk
// (secret-sharing/src/pss.rs:125-166 with T = a curve point, secret-sharing/src/gao.rs for the code).
//   syndromes  S_j = sum_p w_n^(-p j) Y_p, j = k .. n - 1: n times coefficient j of the interpolant.  The word is a codeword
//              of dimension k exactly when all of them are the identity.
//   one error  E at party q gives S_j = w_n^(-q j) E, so S_(j+1) = w_n^(-q) S_j for every j: q is the one candidate for
//              which that holds at j = k (the n multiples w_n^(-q) S_k of a point of order r are distinct), the other
//              syndromes must follow the same ratio, E = w_n^(q k) S_k (the 1 / n of the coefficient never enters), and the honest
//              share is Y_q - E.
// cap = 1 when n - k >= 2, else 0: below Gao's (n - k) / 2, see include/zksaas.h.
//   status 0  all syndromes are the identity
//   status 1  S_k is not the identity and the syndromes are a geometric sequence of ratio w_n^(-q): exactly the words one share
//             away from a codeword.  errpos = 1 << q
//   status 2  anything else
// Two parts, both host + device code (tests/native/gao_points_host_test.cpp runs the text the kernels compile):
//   gao_points_row     one lane, one chunk, one coefficient row: a syndrome, or a secret of the plain unpack (stage 1)
//   gao_points_chunk   n lanes, one dirty chunk (stage 2), written against the lane group of gao.hpp.  A lane takes one
//                      candidate q, then one consistency check or one of the products the output needs; the group agrees by
//                      ballot.  No point crosses lanes.
// With a party list (zk_pss_unpack_points_robust_parties, zk_pss_repair_points_parties) both parts run on the word deflated by
// the absent parties' locator, whose factors sit in a table of scalars per (list, dimension): GaoPtList, further down.
// Stage 2 reads the syndromes stage 1 computed, as affine points: an inversion per syndrome of a dirty chunk only (the
// identity needs none), and the decoder's products are then mixed additions on a base of two coordinates -- an XYZZ base over
// Fq2 of BLS12-381 would be 96 registers on its own.
// Every point addition goes through the complete forms of ec.hpp (equal and opposite operands, the identity); every loop has
// a fixed trip count, so shares outside the precondition (on the curve, in the order-r subgroup) end in a verdict that means
// nothing, and never in a lane that spins.
#pragma once
#include <vector>

#include "ec.hpp"
#include "gao.hpp"

namespace zk {

// Scalars of one packing factor: a small device table, read at run-time indices; a context uploads it once.
template <class F>
struct GaoPtTable {
  F winv[GAO_MAX_N];       // w_n^-e, CANONICAL (what the double-and-add walks read), zero for e >= n
  F wn[GAO_MAX_N];         // w_n^e, Montgomery: a factor of the error's scalar
};
template <class P>
inline GaoPtTable<Fp<P>> gao_points_make_table(int l) {
  using F = Fp<P>;
  const int n = 4 * l;
  const GaoConsts<F> c = gao_make_consts<P>(l);
  GaoPtTable<F> t;
  for (int e = 0; e < GAO_MAX_N; e++) {
    t.winv[e] = e < n ? gao_lane_pow<F, 5>(c.wipow2, e).from_mont() : F::zero();
    t.wn[e] = e < n ? gao_lane_pow<F, 5>(c.wpow2, e) : F::zero();
  }
  return t;
}

// s A for a canonical scalar s: MSB-first double-and-add over all 32 N bits.  The scalar is shifted through its own limbs, so
// no limb is read at a run-time index (a register array indexed by the loop counter goes to scratch memory).
template <class FrP, class Fld>
ZK_HD XYZZ<Fld> gao_pt_mul(const Affine<Fld>& a, const Fp<FrP>& s) {
  constexpr int N = FrP::N;
  XYZZ<Fld> acc = XYZZ<Fld>::identity();
  const bool id = a.is_identity();
  Fp<FrP> k = s;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < 32 * N; i++) {
    acc = xyzz_dbl(acc);
    const bool bit = (k.v[N - 1] >> 31) != 0;
#pragma unroll
    for (int j = N - 1; j > 0; j--) k.v[j] = (k.v[j] << 1) | (k.v[j - 1] >> 31);
    k.v[0] <<= 1;
    if (bit && !id) acc = xyzz_madd(acc, a.x, a.y);
  }
  return acc;
}
// a == b as group elements
template <class Fld>
ZK_HD bool gao_pt_eq(const XYZZ<Fld>& a, const Affine<Fld>& b) {
  if (a.is_identity() || b.is_identity()) return a.is_identity() && b.is_identity();
  return (b.x * a.ZZ - a.X).is_zero() && (b.y * a.ZZZ - a.Y).is_zero();
}
// xyzz_to_affine with every product of a prime coordinate field inline: inverse_fast ends in two out-of-line products, whose
// operands pass through scratch memory (as gao.hpp's decoder found); the quadratic extension keeps its own form
template <class P>
ZK_HD Fp<P> gao_pt_inv(const Fp<P>& x) {
  return x.template inverse_safegcd<true>() * Fp<P>::r2() * Fp<P>::r2();
}
template <class P, bool I>
ZK_HD Fp2T<P, I> gao_pt_inv(const Fp2T<P, I>& x) {
  return x.inverse_fast();
}
template <class Fld>
ZK_HD Affine<Fld> gao_pt_to_affine(const XYZZ<Fld>& p) {
  if (p.is_identity()) return {Fld::zero(), Fld::zero()};
  const Fld zi = gao_pt_inv(p.ZZZ);      // 1 / Z^3
  const Fld zi2 = (zi * p.ZZ).sqr();     // 1 / Z^2
  return {p.X * zi2, p.Y * zi};
}
// a - t in affine form: the mixed addition takes equal operands, opposite operands and an identity accumulator itself
template <class Fld>
ZK_HD Affine<Fld> gao_pt_sub(const Affine<Fld>& a, const XYZZ<Fld>& t) {
  const XYZZ<Fld> nt = t.neg();
  if (a.is_identity()) return gao_pt_to_affine(nt);
  return gao_pt_to_affine(xyzz_madd(nt, a.x, a.y));
}

// a, or the identity: chosen limb by limb.  (`keep ? a : ident` over two addressable points compiles to a select of their
// ADDRESSES, which puts both into scratch memory.)
template <class P>
ZK_HD Fp<P> gao_fld_keep(const Fp<P>& a, bool keep) {
  Fp<P> r;
#pragma unroll
  for (int i = 0; i < P::N; i++) r.v[i] = keep ? a.v[i] : 0u;
  return r;
}
template <class P, bool I>
ZK_HD Fp2T<P, I> gao_fld_keep(const Fp2T<P, I>& a, bool keep) {
  return {gao_fld_keep(a.c0, keep), gao_fld_keep(a.c1, keep)};
}
template <class Fld>
ZK_HD Affine<Fld> gao_pt_keep(const Affine<Fld>& a, bool keep) {
  return {gao_fld_keep(a.x, keep), gao_fld_keep(a.y, keep)};
}

// ---------------------------------------------------------------- stage 1: one lane, one chunk, one row
// sum_p coef(p) Y_p over the n shares ld(p) of the chunk; coef(p): pointer to a canonical scalar in memory.  One doubling
// chain for all n inputs, as points_lincomb_kernel; lanes that share the row take every bit test alike.
template <class FrP, class Fld, class Coef, class Ld>
ZK_HD XYZZ<Fld> gao_points_row(int n, Coef coef, Ld ld) {
  XYZZ<Fld> acc = XYZZ<Fld>::identity();
  for (int w = FrP::N - 1; w >= 0; w--)
    for (int b = 31; b >= 0; b--) {
      acc = xyzz_dbl(acc);
      for (int p = 0; p < n; p++) {
        if (!((coef(p)->v[w] >> b) & 1u)) continue;
        const Affine<Fld> y = ld(p);
        if (!y.is_identity()) acc = xyzz_madd(acc, y.x, y.y);
      }
    }
  return acc;
}
// the scalar of syndrome row i (S_(k+i)) at party p: w_n^(-p (k + i))
template <class F>
ZK_HD const F* gao_points_syn_coef(const GaoPtTable<F>* tab, int n, int k, int i, int p) {
  return &tab->winv[(p * (k + i)) & (n - 1)];
}

// ---------------------------------------------------------------- stage 2: n lanes, one dirty chunk
// The lambdas that hold a scalar multiplication are inlined by attribute: left to the inliner, the 12-limb forms became
// functions of their own, and a point passed to or from a function travels through scratch memory.
#define GAO_PT_INLINE __attribute__((always_inline))
template <class Fld, class G>
struct GaoPtResult {
  int status;                                      // 1 or 2 (a clean chunk never reaches the decoder)
  uint32_t errpos;                                 // 1 << q, or 0
  typename G::template V<Affine<Fld>> val;         // lane i < nfix: base(q, i) - (lane i's multiple of E); identity on failure
};

// One chunk, all n lanes of the group together; a group that is not `live` takes every step with the others.
//   syn(i)       S_(k+i) of this group's chunk, affine, i < nsyn = n - k
//   nfix         how many lanes produce an output (0: the verdict only)
//   RE           zk_pss_repair_points: nfix <= 1, lane 0's output is Y_q - E, base(q, 0) = the share of party q
//   otherwise    lane i's output is secret i of the corrected word, (secret i of the received word) - U[i][q] E:
//                base(q, i) = what stage 1 wrote for secret i, ucoef(i, q) = U[i][q], canonical
// The lanes' work is a list of products of a syndrome by a scalar: first the nfix multiples of S_k the outputs need, then
// the checks w^(-q) S_(k+c) == S_(k+c+1), c = 1 .. n - k - 2; the list is walked n tasks at a time.
// k is the dimension the decoder runs at on the full domain and enters through nsyn = n - k only; the all-party form and the
// party-list form below differ in who may be a candidate and in the error's scalar:
//   listed(p)    party p may be named (all n parties: always)
//   escal(q)     E = escal(q) S_k, Montgomery (all n parties: w^(q k))
template <class FrP, class Fld, class G, bool RE, class Syn, class Base, class UCoef, class Listed, class ErrScal>
ZK_HD GaoPtResult<Fld, G> gao_points_chunk_on(const G& g, const GaoPtTable<Fp<FrP>>* tab, int n, int nsyn, int nfix, bool live,
                                              Syn syn, Base base, UCoef ucoef, Listed listed, ErrScal escal) {
  using Fr = Fp<FrP>;
  using A = Affine<Fld>;
  using P = XYZZ<Fld>;
  using VP = typename G::template V<P>;
  using VA = typename G::template V<A>;
  const A ident{Fld::zero(), Fld::zero()};
  bool ok = live && nsyn >= 2;
  int q = 0;
  VA val = g.template make<A>([&](int) { return ident; });
  if (g.wave_any(ok)) {
    // ---- locate: lane p asks whether w^(-p) S_k == S_(k+1)
    const A s0 = syn(0), s1 = syn(1);
    const VP cand = g.template make<P>([&](int p) GAO_PT_INLINE { return gao_pt_mul<FrP, Fld>(s0, tab->winv[p]); });
    const uint32_t m = g.ballot([&](int p) { return listed(p) && gao_pt_eq(g.at(cand, p), s1); });
    if (s0.is_identity() || gao_popcount(m) != 1) ok = false;
    q = ok ? gao_top_bit(m) : 0;
    // ---- the outputs' products and the consistency checks
    const int ntask = nfix + nsyn - 2;
    const Fr es = escal(q);
    for (int t0 = 0; t0 < ntask; t0 += n) {
      const VP pr = g.template make<P>([&](int p) GAO_PT_INLINE {
        const int t = t0 + p;
        const bool fix = t < nfix, chk = !fix && t < ntask;
        Fr s = tab->winv[q];
        if (fix) {
          if constexpr (RE) s = es.from_mont();
          else s = (ucoef(t, q).to_mont() * es).from_mont();
        }
        return gao_pt_mul<FrP, Fld>(syn(chk ? t - nfix + 1 : 0), s);
      });
      const uint32_t bad = g.ballot([&](int p) {
        const int t = t0 + p;
        return t >= nfix && t < ntask && !gao_pt_eq(g.at(pr, p), syn(t - nfix + 2));
      });
      if (bad) ok = false;
      if (t0 == 0)
        val = g.template make<A>([&](int p) GAO_PT_INLINE {
          A v{Fld::zero(), Fld::zero()};
          if (p < nfix) v = gao_pt_sub(base(q, p), g.at(pr, p));
          return v;
        });
    }
  }
  GaoPtResult<Fld, G> out;
  out.status = ok ? 1 : 2;
  out.errpos = ok ? 1u << q : 0;
  out.val = g.template make<A>([&](int p) { return gao_pt_keep(g.at(val, p), ok); });
  return out;
}
// the error's scalar with all n parties: w^(q k)
template <class F>
ZK_HD F gao_points_err_scalar(const GaoPtTable<F>* tab, int n, int k, int q) {
  return tab->wn[(q * k) & (n - 1)];
}
template <class FrP, class Fld, class G, bool RE, class Syn, class Base, class UCoef>
ZK_HD GaoPtResult<Fld, G> gao_points_chunk(const G& g, const GaoPtTable<Fp<FrP>>* tab, int n, int k, int nfix, bool live, Syn syn,
                                           Base base, UCoef ucoef) {
  return gao_points_chunk_on<FrP, Fld, G, RE>(
      g, tab, n, n - k, nfix, live, syn, base, ucoef, [](int) { return true; },
      [&](int q) { return gao_points_err_scalar(tab, n, k, q); });
}

// ---------------------------------------------------------------- a party list (zk_pss_*_points_*_parties)
// With the parties of a set S listed (np of them, compact rows in ascending id), rho = n - np absent and
// Lambda(X) = prod_{a not in S} (X - w_n^a), the deflated word Y'_p = Lambda(w_n^p) Y_p for p in S, the identity otherwise, is a
// word of dimension k' = k + rho on the full domain: gao_make_absent's device, carried into the exponent.  A lane never
// multiplies a point by Lambda on its own -- the factor sits in the scalars it reads:
//   syndromes  S_j = sum_{p in S} Lambda(w_n^p) w_n^(-p j) Y_p, j = k' .. n - 1: np - k rows over the compact shares
//   one error  E at a listed q: S_(j+1) = w_n^(-q) S_j as before, E = Lambda(w_n^q)^(-1) w_n^(q k') S_k'
// Only listed parties are candidates; a ratio that points at an absent party is status 2, as in gao.hpp.  cap = 1 when
// np - k >= 2, else 0.  The secrets go through the l x np Lagrange matrix of the listed points at g w_2l^i, valid for any word
// of dimension <= np.  Everything here depends on (list, k) only and is computed on the host.
template <class F>
struct GaoPtList {         // a view: device pointers in a kernel, host pointers in the host test
  const uint32_t* row;     // [n] party p's row of the compact shares; 0 for an absent one, which is never named
  const F* fix;            // [n] Lambda(w_n^q)^(-1) w_n^(q k'), Montgomery; zero for an absent q
  const F* syn;            // [np - k][np] Lambda(w_n^p) w_n^(-p (k' + i)) at p's row, CANONICAL
  const F* umat;           // [l][np] the Lagrange matrix, CANONICAL
  int np, kp;              // listed parties; k' = k + rho
  uint32_t listed;         // bit p: party p is listed
};
constexpr size_t GAO_PT_LIST_HEAD = GAO_MAX_N * sizeof(uint32_t);      // `row`, ahead of the scalars in one allocation
template <class F>
struct GaoPtListHost {
  uint32_t row[GAO_MAX_N];
  std::vector<F> sc;       // fix [n] | syn [np - k][np] | umat [l][np]
  int n, l, np, kp;
  uint32_t listed;
  size_t bytes() const { return GAO_PT_LIST_HEAD + sc.size() * sizeof(F); }
  // the view of a copy that starts at `base`: row, then sc
  GaoPtList<F> view(const void* base) const {
    const F* s = (const F*)((const char*)base + GAO_PT_LIST_HEAD);
    return {(const uint32_t*)base, s, s + n, s + n + (size_t)(n - kp) * np, np, kp, listed};
  }
  GaoPtList<F> view() const { return {row, sc.data(), sc.data() + n, sc.data() + n + (size_t)(n - kp) * np, np, kp, listed}; }
};
// parties: np ascending ids below n = 4l (null: 0 .. np - 1), np > k
template <class P>
inline GaoPtListHost<Fp<P>> gao_points_make_list(int l, const uint32_t* parties, int np, int k) {
  using F = Fp<P>;
  const int n = 4 * l, rho = n - np, kp = k + rho, nsyn = np - k;
  const GaoConsts<F> c = gao_make_consts<P>(l);
  GaoPtListHost<F> t;
  t.n = n, t.l = l, t.np = np, t.kp = kp, t.listed = 0;
  uint32_t ids[GAO_MAX_N];
  for (int i = 0; i < GAO_MAX_N; i++) t.row[i] = 0;
  for (int i = 0; i < np; i++) ids[i] = parties ? parties[i] : (uint32_t)i, t.row[ids[i]] = (uint32_t)i, t.listed |= 1u << ids[i];
  F x[GAO_MAX_N], lam[GAO_MAX_N];
  for (int p = 0; p < n; p++) x[p] = gao_lane_pow<F, 5>(c.wpow2, p);
  for (int p = 0; p < n; p++) {
    lam[p] = F::one();
    for (int a = 0; a < n; a++)
      if (!((t.listed >> a) & 1)) lam[p] = lam[p] * (x[p] - x[a]);
  }
  t.sc.assign((size_t)n + (size_t)nsyn * np + (size_t)l * np, F::zero());
  F* fix = t.sc.data();
  F* syn = fix + n;
  F* um = syn + (size_t)nsyn * np;
  for (int i = 0; i < np; i++) {
    const int q = (int)ids[i];
    fix[q] = lam[q].inverse() * x[(q * kp) & (n - 1)];
    for (int r = 0; r < nsyn; r++) syn[(size_t)r * np + i] = (lam[q] * x[(n - ((q * (kp + r)) & (n - 1))) & (n - 1)]).from_mont();
    for (int s = 0; s < l; s++) {
      F num = F::one(), den = F::one();
      for (int j = 0; j < np; j++)
        if (j != i) num = num * (c.sec[s] - x[ids[j]]), den = den * (x[q] - x[ids[j]]);
      um[(size_t)s * np + i] = (num * den.inverse()).from_mont();
    }
  }
  return t;
}
// gao_points_chunk for a party list; base and ucoef take the party id q and look its row up in lt.row
template <class F>
ZK_HD bool gao_points_listed(const GaoPtList<F>& lt, int p) {
  return ((lt.listed >> p) & 1u) != 0;
}
template <class FrP, class Fld, class G, bool RE, class Syn, class Base, class UCoef>
ZK_HD GaoPtResult<Fld, G> gao_points_chunk_parties(const G& g, const GaoPtTable<Fp<FrP>>* tab, const GaoPtList<Fp<FrP>>& lt, int n,
                                                   int nfix, bool live, Syn syn, Base base, UCoef ucoef) {
  return gao_points_chunk_on<FrP, Fld, G, RE>(
      g, tab, n, n - lt.kp, nfix, live, syn, base, ucoef, [&](int p) { return gao_points_listed(lt, p); },
      [&](int q) { return lt.fix[q]; });
}

#undef GAO_PT_INLINE

#if defined(__HIPCC__)
class IEngine;
struct DevBuf;
// zk_pss_unpack_points_robust (REPAIR = false; umat: the l x n unpack matrix, canonical, device; out may be null) and
// zk_pss_repair_points (REPAIR = true; shares written, umat and out null) over the coordinate field Fld; tab: the device
// copy of gao_points_make_table(l); wk: working memory.  list (null: all n parties): a view of device memory for the
// _parties forms -- shares are its np rows, the matrix is its own and umat is not read
template <class FrP, class Fld, bool REPAIR>
int gao_points_run(IEngine* e, DevBuf& wk, int l, std::conditional_t<REPAIR, void*, const void*> shares, size_t nchunks,
                   int dimension, const GaoPtTable<Fp<FrP>>* tab, const Fp<FrP>* umat, const GaoPtList<Fp<FrP>>* list, void* out,
                   uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st);
#endif

}  // namespace zk
