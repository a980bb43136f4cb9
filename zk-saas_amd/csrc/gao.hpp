// Error-correcting unpack (zk_pss_unpack_robust): bounded-distance decoding of the Reed-Solomon word the n = 4l shares of one
// chunk form, after secret-sharing/src/gao.rs:11-84 (partial_xgcd, decode_to_message) with the early return and the failure
// checks its todo lines ask for.  For a received word y on the share domain H_n and a dimension k, cap = (n - k) / 2:
//   status 0  the interpolant R = IFFT(y) has degree < k                                  -> h = R
//   status 1  a polynomial h of degree < k agrees with y in all but 1 .. cap positions    -> h, the positions in errpos
//   status 2  neither                                                                     -> zeros
// Two parts, both host + device code (tests/native/gao_host_test.cpp runs the text the kernels compile):
//   gao_load / gao_ifft / gao_is_clean / gao_clean_secrets   one lane (two at l = 8), one chunk: the syndrome test and the
//                                                 clean unpack (stage 1)
//   gao_chunk                                     n lanes, one chunk: Gao's decoder (stage 2), written against a lane group
// zk_pss_repair runs the same two parts without secrets and message: stage 1 up to gao_is_clean (the scan), and the decoder
// with its flag RE, whose re-encoding h(w_n^p) replaces the share of every party named in errpos (section "repair" below;
// tests/native/gao_repair_host_test.cpp runs that text).
// The lane group G gives the decoder its cross-lane operations -- broadcast from a lane, shift by d lanes, ballot, any -- with
// a value of type G::V<T> holding one T per lane: GaoDevGroup (gao_impl.hpp) maps them to the wave's cross-lane builtins and
// V<T> = T, GaoHostGroup below is a loop over an array of n lanes.  Lane p holds coefficient p of a polynomial.
// zk_pss_unpack_robust_parties -- the shares of a party list, the others absent -- runs the same two parts on a word made
// full-length again: the section "absent parties" below (tests/native/gao_erasure_host_test.cpp runs that text), and
// zk_pss_repair_parties is its repair form (tests/native/gao_repair_parties_host_test.cpp).
// Every public form -- all parties or a list, unpack or repair, one word, a batch of words or a word in a block with padding
// -- is ONE description of a call (GaoCall, the last section) handed to ONE host driver, gao_run<FrP, REPAIR> (gao_impl.hpp):
// its refusals (gao_list_check, gao_call_check) and its working memory (gao_layout) are host text below.
#pragma once
#include <type_traits>

#include "../../include/zksaas.h"
#include "field.hpp"
#include "king_range.hpp"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace zk {

constexpr int GAO_MAX_N = 32;

// Constants of one packing factor.  A kernel takes them by value and reads them at compile-time indices only.
template <class F>
struct GaoConsts {
  F ninv;                  // 1 / n
  F tw[GAO_MAX_N / 2];     // w_n^-j, j < n / 2: the twiddles of the inverse transform over H_n
  F wpow2[5], wipow2[5];   // w_n^(2^b), w_n^-(2^b)
  F spow2[3];              // w_2l^(2^b)
  F g;                     // the coset generator
  F sec[8];                // g w_2l^i, i < l: where the secrets sit (pss.rs:44-52)
};

template <class P>
inline GaoConsts<Fp<P>> gao_make_consts(int l) {
  using F = Fp<P>;
  const int n = 4 * l;
  auto root = [](int size) {
    F r = F::from_limbs(P::TWO_ADIC_ROOT);
    for (int i = 0; ((size_t)size << i) < ((size_t)1 << P::TWO_ADICITY); i++) r = r.sqr();
    return r;
  };
  GaoConsts<F> c;
  const F z = F::zero();
  c.ninv = F::from_u64((uint64_t)n).inverse();
  const F w = root(n), wi = w.inverse(), w2l = l == 1 ? (z - F::one()) : root(2 * l);
  F cur = F::one();
  for (int j = 0; j < GAO_MAX_N / 2; j++) c.tw[j] = j < n / 2 ? cur : z, cur = cur * wi;
  F a = w, b = wi, s = w2l;
  for (int i = 0; i < 5; i++) c.wpow2[i] = a, c.wipow2[i] = b, a = a.sqr(), b = b.sqr();
  for (int i = 0; i < 3; i++) c.spow2[i] = s, s = s.sqr();
  c.g = F::from_limbs(P::GENERATOR);
  cur = c.g;
  for (int i = 0; i < 8; i++) c.sec[i] = i < l ? cur : z, cur = cur * w2l;
  return c;
}

// base^e for e < 2^NB from the squarings pow2[b] = base^(2^b)
template <class F, int NB>
ZK_HD F gao_lane_pow(const F* pow2, int e) {
  F r = F::one();
#pragma unroll
  for (int b = 0; b < NB; b++)
    if ((e >> b) & 1) r = r * pow2[b];
  return r;
}

// ---------------------------------------------------------------- stage 1: one lane (or two), one chunk
// A chunk is worked on by SP = 1 or 2 lanes.  With SP = 2 (l = 8: 32 coefficients of 8 limbs do not fit one lane's registers)
// lane q takes the first decimation-in-frequency stage at the load -- y_i + y_{i+n/2}, or (y_i - y_{i+n/2}) w^-i -- and then
// holds the M = n / 2 coefficients of index 2 j' + q.  In general a lane holds coefficient SP j' + q at x[gao_bitrev(j', M)].
constexpr int gao_split(int l) { return l >= 8 ? 2 : 1; }
constexpr int gao_bitrev(int i, int n) {
  int r = 0;
  for (int b = 1; b < n; b <<= 1) r = (r << 1) | ((i & b) ? 1 : 0);
  return r;
}
constexpr int gao_log2(int n) { return n <= 1 ? 0 : 1 + gao_log2(n / 2); }
// fn(integral_constant<int, I>) for I = B .. E - 1: the loops of the one-lane form, unrolled by the language and not by a
// pragma -- with products inline the bodies are large, the unroller left the outer loops rolled and the array of loaded
// elements, then indexed at run time, went to scratch memory
template <int B, int E, class Fn>
ZK_HD void gao_static_for(Fn&& fn) {
  if constexpr (B < E) {
    fn(std::integral_constant<int, B>{});
    gao_static_for<B + 1, E>(fn);
  }
}
// x[i], i < M, from the shares ld(p), p < SP M, for lane q of the split
template <int M, int SP, class F, class Ld>
ZK_HD void gao_load(const GaoConsts<F>& c, int q, Ld ld, F* x) {
  gao_static_for<0, M>([&](auto i_) {
    constexpr int i = decltype(i_)::value;
    if constexpr (SP == 1) {
      x[i] = ld(i);
    } else {
      const F u = ld(i), v = ld(i + M);
      if constexpr (i == 0) x[i] = q ? u - v : u + v;
      else x[i] = q ? (u - v) * c.tw[i] : u + v;
    }
  });
}
// In place: x[gao_bitrev(j', M)] = n R_{SP j' + q}, R = IFFT_{H_n}(y).  Radix 2, decimation in frequency, every index a
// compile-time constant: (M / 2) (log2 M - 1) - (M / 2 - 1) products -- 1, 5, 17 for M = 4, 8, 16.
template <int M, int SP, class F>
ZK_HD void gao_ifft(const GaoConsts<F>& c, F* x) {
  gao_static_for<0, gao_log2(M)>([&](auto s_) {
    gao_static_for<0, M / 2>([&](auto t_) {
      constexpr int s = decltype(s_)::value, t = decltype(t_)::value;
      constexpr int len = M >> s, h = len / 2, i = t % h, lo = (t / h) * len + i;
      const F u = x[lo], v = x[lo + h];
      x[lo] = u + v;
      if constexpr (i == 0) x[lo + h] = u - v;
      else x[lo + h] = (u - v) * c.tw[(i << s) * SP];
    });
  });
}
// this lane's coefficients of index >= k all zero
template <int M, int SP, class F>
ZK_HD bool gao_is_clean(const F* x, int k, int q) {
  bool clean = true;
  gao_static_for<0, M>([&](auto j_) {
    constexpr int j = decltype(j_)::value;
    if (SP * j + q >= k && !x[gao_bitrev(j, M)].is_zero()) clean = false;
  });
  return clean;
}
// put(j, R_j) for this lane's j < k: the message of a clean word
template <int M, int SP, class F, class Put>
ZK_HD void gao_clean_message(const GaoConsts<F>& c, const F* x, int k, int q, Put put) {
  gao_static_for<0, M>([&](auto j_) {
    constexpr int j = decltype(j_)::value;
    if (SP * j + q < k) put(SP * j + q, x[gao_bitrev(j, M)] * c.ninv);
  });
}
// put(i, this lane's part of R(g w_2l^i)), i < l, for R of degree < k: Horner over the coefficients the transform left (in
// X^SP, lane 1 of a split then multiplies by X), then the 1 / n; the parts of the SP lanes add up to the secret.
// Every multiply is inline (an out-of-line one passes its operands through scratch memory, and the values that live across a
// call no longer fit the registers a callee preserves).  For l >= 4 the secrets are a loop that is not unrolled, so the
// products of one evaluation are in the code once: the coefficient indices stay compile-time constants, the loop index only
// moves the point on by one product and selects where put() stores.
// The last product of a secret is by scale(i): 1 / n here, 1 / (n Lambda(g w_2l^i)) with absent parties (below).  For l >= 4
// i is a run-time index: scale() must not read by-value constants there.
template <int M, int SP, class F, class Scale, class Put>
ZK_HD void gao_clean_secrets(const GaoConsts<F>& c, const F* x, int k, int q, Scale scale, Put put) {
  constexpr int L = M * SP / 4;
  if constexpr (L <= 2) {
    static_assert(SP == 1, "no split at small l");
    F sec[L];
    gao_static_for<0, L>([&](auto i_) { sec[decltype(i_)::value] = F::zero(); });
    gao_static_for<0, M>([&](auto r_) {
      constexpr int j = M - 1 - decltype(r_)::value;
      if (j < k) gao_static_for<0, L>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        sec[i] = sec[i] * c.sec[i] + x[gao_bitrev(j, M)];
      });
    });
    gao_static_for<0, L>([&](auto i_) { put(decltype(i_)::value, sec[decltype(i_)::value] * scale(decltype(i_)::value)); });
  } else {
    F pt1 = c.g;              // g w_2l^i, walked: a run-time index into the constants would copy them to scratch memory
#pragma unroll 1
    for (int i = 0; i < L; i++) {
      if (i) pt1 = pt1 * c.spow2[0];
      const F pt = SP == 1 ? pt1 : pt1.sqr();
      F acc = F::zero();
      gao_static_for<0, M>([&](auto r_) {
        constexpr int j = M - 1 - decltype(r_)::value;
        if (SP * j + q < k) acc = acc * pt + x[gao_bitrev(j, M)];
      });
      if (SP == 2 && q) acc = acc * pt1;
      put(i, acc * scale(i));
    }
  }
}
template <int M, int SP, class F, class Put>
ZK_HD void gao_clean_secrets(const GaoConsts<F>& c, const F* x, int k, int q, Put put) {
  gao_clean_secrets<M, SP>(c, x, k, q, [&](int) -> const F& { return c.ninv; }, put);
}

// ---------------------------------------------------------------- the host lane group
struct GaoHostGroup {
  template <class T>
  struct V {
    T a[GAO_MAX_N];
  };
  int n;
  template <class T>
  const T& at(const V<T>& v, int p) const { return v.a[p]; }
  template <class T, class Fn>
  V<T> make(Fn fn) const {
    V<T> o{};
    for (int p = 0; p < n; p++) o.a[p] = fn(p);
    return o;
  }
  template <class T>
  T bcast(const V<T>& v, int src) const { return v.a[src]; }
  template <class T>
  V<T> shift(const V<T>& v, int d) const {
    V<T> o{};
    for (int p = 0; p < n; p++) o.a[p] = p >= d ? v.a[p - d] : T::zero();
    return o;
  }
  template <class Fn>
  uint32_t ballot(Fn pred) const {
    uint32_t m = 0;
    for (int p = 0; p < n; p++)
      if (pred(p)) m |= 1u << p;
    return m;
  }
  bool wave_any(bool b) const { return b; }
};

// ---------------------------------------------------------------- stage 2: n lanes, one chunk
// index of the highest set bit, -1 for 0: the degree of a polynomial from the ballot of its nonzero coefficients
ZK_HD int gao_top_bit(uint32_t m) { return m ? 31 - __builtin_clz(m) : -1; }
ZK_HD int gao_popcount(uint32_t m) { return __builtin_popcount(m); }

// RE (zk_pss_repair): the result also carries the re-encoding h(w_n^p) every lane computes for the comparison with its share,
// and the secrets are not evaluated.  A flag and not a member of every result: the unpack kernels keep their registers.
template <class VF, bool RE>
struct GaoReencoding {};
template <class VF>
struct GaoReencoding<VF, true> {
  VF ev;                               // lane p: h(w_n^p), zero on failure
};
template <class F, class G, bool RE = false>
struct GaoResult : GaoReencoding<typename G::template V<F>, RE> {
  int status;                          // 1 or 2 (a clean word never reaches the decoder)
  uint32_t errpos;
  typename G::template V<F> h;         // lane j: coefficient j of the message, zero for j >= k and on failure
  typename G::template V<F> sec;       // lane i < l: secret i (zero with RE)
};

// One chunk, all n lanes of the group together.  y: lane p holds share p; xp, xinv: w_n^p and w_n^-p; sp: g w_2l^p (read in
// lanes p < l).  A group that is not `live` takes every cross-lane step with the others and changes nothing.
//
// partial_xgcd runs as elementary row operations on [A; SA] (the row being reduced) and [B; SB] (the divisor):
//   [A; SA] <- lc(B) [A; SA] - lc(A) X^d [B; SB],  d = deg A - deg B,
// and a swap once deg A < deg B: one reference loop iteration is the run of steps between two swaps.  A row is the reference's
// row times a nonzero scalar, which h = r / s does not see, so the only inversion is the one of the final exact division.
// z = X^n - 1 has n + 1 coefficients: the first step is taken in closed form, lc(R) z - X^(n - deg R) R, whose X^n terms cancel.
// Every loop has a static bound and runs while any group of the wave is active, so no cross-lane read sits in divergent code
// and no share vector makes the decoder spin.
template <class F, class G, bool RE = false>
ZK_HD GaoResult<F, G, RE> gao_chunk(const G& g, const GaoConsts<F>& c, int n, int k, bool live,
                                const typename G::template V<F>& y, const typename G::template V<F>& xp,
                                const typename G::template V<F>& xinv, const typename G::template V<F>& sp) {
  using VF = typename G::template V<F>;
  const int stop = (n + k) / 2, cap = (n - k) / 2;
  auto deg = [&](const VF& v) { return gao_top_bit(g.ballot([&](int p) { return !g.at(v, p).is_zero(); })); };
  const F zero = F::zero(), one = F::one();
  // ---- R = IFFT(y): lane p evaluates (1 / n) sum_q y_q (w^-p)^q by Horner
  VF B = g.template make<F>([&](int) { return zero; });
  for (int q = n - 1; q >= 0; q--) {
    const F yq = g.bcast(y, q);
    B = g.template make<F>([&](int p) { return g.at(B, p) * g.at(xinv, p) + yq; });
  }
  B = g.template make<F>([&](int p) { return g.at(B, p) * c.ninv; });
  VF SB = g.template make<F>([&](int p) { return p == 0 ? one : zero; });
  // ---- partial_xgcd(z, R): stop at the first remainder of degree < (n + k) / 2
  int degB = deg(B);
  bool active = live && degB >= stop;
  VF A, SA;
  {
    const int d = active ? n - degB : 0;
    const F lc = g.bcast(B, degB < 0 ? 0 : degB);
    const VF sh = g.shift(B, d);
    A = g.template make<F>([&](int p) { return p == 0 ? zero - g.at(sh, p) - lc : zero - g.at(sh, p); });
    SA = g.template make<F>([&](int p) { return p == d ? zero - one : zero; });
  }
  for (int it = 0; it < 2 * n + 2; it++) {
    if (!g.wave_any(active)) break;
    int degA = deg(A);
    degB = deg(B);
    const bool sw = active && degA < degB;
    {
      const VF tA = A, tS = SA;
      A = g.template make<F>([&](int p) { return sw ? g.at(B, p) : g.at(tA, p); });
      B = g.template make<F>([&](int p) { return sw ? g.at(tA, p) : g.at(B, p); });
      SA = g.template make<F>([&](int p) { return sw ? g.at(SB, p) : g.at(tS, p); });
      SB = g.template make<F>([&](int p) { return sw ? g.at(tS, p) : g.at(SB, p); });
    }
    if (sw) {
      const int t = degA;
      degA = degB, degB = t;
    }
    if (active && degB < stop) active = false;
    const int d = active ? degA - degB : 0;
    const F a = g.bcast(B, degB < 0 ? 0 : degB), b = g.bcast(A, degA < 0 ? 0 : degA);
    const VF shB = g.shift(B, d), shS = g.shift(SB, d);
    const bool on = active;
    A = g.template make<F>([&](int p) { return on ? a * g.at(A, p) - b * g.at(shB, p) : g.at(A, p); });
    SA = g.template make<F>([&](int p) { return on ? a * g.at(SA, p) - b * g.at(shS, p) : g.at(SA, p); });
  }
  // a group still active here has met the static bound, which no input reaches: it fails
  bool ok = live && !active;
  // ---- h = r / s, exactly, with deg h < k (decode_to_message's divide_with_q_and_r and its assert)
  const int dr = deg(B), ds = deg(SB), qd = dr - ds;
  if (qd >= k || ds < 0) ok = false;
  const F inv = g.bcast(SB, ds < 0 ? 0 : ds).template inverse_safegcd<true>() * F::r2() * F::r2();
  VF rem = B, h = g.template make<F>([&](int) { return zero; });
  for (int j = k - 1; j >= 0; j--) {
    const bool on = ok && j <= qd;
    const F q = g.bcast(rem, on ? ds + j : 0) * inv;
    const VF sh = g.shift(SB, j);
    rem = g.template make<F>([&](int p) { return on ? g.at(rem, p) - q * g.at(sh, p) : g.at(rem, p); });
    h = g.template make<F>([&](int p) { return on && p == j ? q : g.at(h, p); });
  }
  if (g.ballot([&](int p) { return !g.at(rem, p).is_zero(); })) ok = false;
  // ---- re-encode: lane p compares h(w^p) with its own share; lanes i < l evaluate the secrets
  VF ev = g.template make<F>([&](int) { return zero; }), sv = ev;
  for (int j = k - 1; j >= 0; j--) {
    const F hj = g.bcast(h, j);
    ev = g.template make<F>([&](int p) { return g.at(ev, p) * g.at(xp, p) + hj; });
    if constexpr (!RE) sv = g.template make<F>([&](int p) { return g.at(sv, p) * g.at(sp, p) + hj; });
  }
  const uint32_t diff = g.ballot([&](int p) { return g.at(ev, p) != g.at(y, p); });
  if (gao_popcount(diff) > cap) ok = false;
  GaoResult<F, G, RE> out;
  if constexpr (RE) out.ev = g.template make<F>([&](int p) { return ok ? g.at(ev, p) : zero; });
  out.status = ok ? 1 : 2;
  out.errpos = ok ? diff : 0;
  out.h = g.template make<F>([&](int p) { return ok ? g.at(h, p) : zero; });
  out.sec = g.template make<F>([&](int p) { return ok ? g.at(sv, p) : zero; });
  return out;
}

// ---------------------------------------------------------------- repair (zk_pss_repair)
// What the decoder's verdict does to the received word, lane by lane: put(p, h(w_n^p)) for every party p named in the errpos
// of a corrected chunk.  A failed chunk has errpos 0 and a clean one never reaches the decoder: nothing else is written.
template <class F, class G, class Put>
ZK_HD void gao_repair_word(const G& g, const GaoResult<F, G, true>& r, Put put) {
  g.template make<int>([&](int p) {
    if (r.status == 1 && ((r.errpos >> p) & 1)) put(p, g.at(r.ev, p));
    return 0;
  });
}

// ---------------------------------------------------------------- absent parties (zk_pss_unpack_robust_parties)
// With the parties of a set S listed, rho = n - |S| absent and Lambda(X) = prod_{e not in S} (X - w_n^e), the full-length word
//   y~_p = y_p Lambda(w_n^p) for p in S,  0 otherwise
// has IFFT(y~) = R_S Lambda exactly (R_S: the interpolant through S), and a polynomial h of degree < k within e places of y
// on S is h Lambda of degree < k + rho within the same e places of y~.  So both stages run as above at dimension k + rho,
// whose cap (n - k - rho) / 2 is (|S| - k) / 2, on shares multiplied as they are loaded; what comes out is h' = h Lambda:
//   secrets  h'(g w_2l^i) / Lambda(g w_2l^i)      the points lie outside H_n, no denominator is zero
//   message  h' / Lambda, an exact division       one lane: root by root (gao_deflate); a lane group: by the monic Lambda
//   status 1 naming an absent party becomes status 2: by the distance of the (k + rho)-code no h exists then
// Everything here depends on the party list only and is computed on the host per call.
template <class F>
struct GaoAbsentLoad {     // stage 1 takes this by value and reads it at compile-time indices only
  F lam[GAO_MAX_N];        // Lambda(w_n^p) for a listed party p, zero for an absent one
  int row[GAO_MAX_N];      // party p's row of shares_d, -1 for an absent one
};
template <class F>
struct GaoAbsent {         // a small device table: what is read at a run-time index
  GaoAbsentLoad<F> ld;
  F lamc[GAO_MAX_N];       // the coefficients of Lambda (monic, degree rho), zero beyond
  F root[GAO_MAX_N];       // w_n^e for the absent parties e, rho of them
  F sscale[8];             // 1 / (n Lambda(g w_2l^i))
  F slam[8];               // 1 / Lambda(g w_2l^i)
  int k, rho;              // the caller's dimension; the decoder runs at k + rho
  uint32_t listed;         // bit p: party p is listed
};

// parties: np ascending ids below n = 4l, np > k
template <class P>
inline GaoAbsent<Fp<P>> gao_make_absent(const GaoConsts<Fp<P>>& c, int l, const uint32_t* parties, int np, int k) {
  using F = Fp<P>;
  const int n = 4 * l;
  GaoAbsent<F> a;
  const F z = F::zero();
  a.k = k, a.rho = n - np, a.listed = 0;
  for (int i = 0; i < GAO_MAX_N; i++) a.ld.lam[i] = a.lamc[i] = a.root[i] = z, a.ld.row[i] = -1;
  for (int i = 0; i < np; i++) a.ld.row[parties[i]] = i, a.listed |= 1u << parties[i];
  a.lamc[0] = F::one();
  int deg = 0;
  for (int e = 0; e < n; e++)
    if (!((a.listed >> e) & 1)) {
      const F r = gao_lane_pow<F, 5>(c.wpow2, e);
      a.root[deg++] = r;
      for (int j = deg; j >= 0; j--) a.lamc[j] = (j ? a.lamc[j - 1] : z) - r * a.lamc[j];      // times (X - r)
    }
  auto lambda_at = [&](const F& x) {
    F v = F::one();
    for (int j = 0; j < a.rho; j++) v = v * (x - a.root[j]);
    return v;
  };
  for (int p = 0; p < n; p++)
    if ((a.listed >> p) & 1) a.ld.lam[p] = lambda_at(gao_lane_pow<F, 5>(c.wpow2, p));
  for (int i = 0; i < 8; i++) {
    a.slam[i] = i < l ? lambda_at(c.sec[i]).inverse() : z;
    a.sscale[i] = a.slam[i] * c.ninv;
  }
  return a;
}

// x <- x / (X - r), exactly, for the coefficients a lane holds (stage 1's layout): b_{j-1} = a_j + r b_j from the top.
// With SP = 2 a lane holds every second coefficient, b_i = a_{i+1} + r a_{i+2} + r^2 b_{i+2}: a_{i+1} is the other lane's,
// one exchange per step -- xch(m, v) is the partner's v of step m (lane 0 sends its a_{2m+2}, lane 1 its a_{2m+1}).
template <int M, int SP, class F, class Xch>
ZK_HD void gao_deflate(F* x, const F& r, int q, Xch xch) {
  if constexpr (SP == 1) {
    F b = F::zero();
    gao_static_for<0, M>([&](auto t_) {
      constexpr int s = gao_bitrev(M - 1 - decltype(t_)::value, M);
      const F a = x[s];
      x[s] = b;
      if constexpr (decltype(t_)::value == 0) b = a;
      else b = a + r * b;
    });
  } else {
    const F r2 = r.sqr();
    F pa = F::zero(), pb = F::zero();
    gao_static_for<0, M>([&](auto t_) {
      constexpr int m = M - 1 - decltype(t_)::value, s = gao_bitrev(m, M);
      const F a = x[s];
      const F got = xch(m, q ? a : pa);
      if constexpr (decltype(t_)::value == 0) x[s] = got;
      else x[s] = got + r * pa + r2 * pb;
      pa = a, pb = x[s];
    });
  }
}

// Stage 2's result for the word y~ (h' = h Lambda, errpos over all n places) -> the result for the listed shares.  slam: lane
// i < l holds 1 / Lambda(g w_2l^i); lamc: lane j holds coefficient j of Lambda.  All lanes of the wave take every cross-lane
// step; k division steps by the monic Lambda, and only when the message is wanted.
// RE (zk_pss_repair_parties): errpos is masked against the list and the verdict demoted as above; the secrets are not scaled
// and h' is not divided -- what the repair needs is ev, lane p's h'(w_n^p) = h(w_n^p) Lambda(w_n^p), zeroed on a demotion.
template <class F, class G, bool RE = false>
ZK_HD void gao_absent_finish(const G& g, int k, int rho, uint32_t listed, bool want_message,
                             const typename G::template V<F>& slam, const typename G::template V<F>& lamc,
                             GaoResult<F, G, RE>& r) {
  using VF = typename G::template V<F>;
  const F zero = F::zero();
  const bool ok = r.status != 2 && !(r.errpos & ~listed);
  r.status = ok ? r.status : 2;
  r.errpos = ok ? r.errpos : 0;
  if constexpr (RE) {
    r.ev = g.template make<F>([&](int p) { return ok ? g.at(r.ev, p) : zero; });
  } else {
    r.sec = g.template make<F>([&](int p) { return ok ? g.at(r.sec, p) * g.at(slam, p) : zero; });
    VF rem = g.template make<F>([&](int p) { return ok ? g.at(r.h, p) : zero; });
    VF h = g.template make<F>([&](int) { return zero; });
    if (want_message)
      for (int j = k - 1; j >= 0; j--) {
        const F q = g.bcast(rem, rho + j);
        const VF sh = g.shift(lamc, j);
        rem = g.template make<F>([&](int p) { return g.at(rem, p) - q * g.at(sh, p); });
        h = g.template make<F>([&](int p) { return p == j ? q : g.at(h, p); });
      }
    r.h = h;
  }
}

// ---------------------------------------------------------------- repair with a party list (zk_pss_repair_parties)
// The decoder's re-encoding of y~ is h'(w_n^p) = h(w_n^p) Lambda(w_n^p); the share to write is that times 1 / Lambda(w_n^p).
// The n inverses are the one table the repair adds: a device table of its own (GaoAbsent travels as a launch argument and
// has no room), read at a run-time index by the lanes that store.
template <class F>
struct GaoInvLambda {
  F v[GAO_MAX_N];          // 1 / Lambda(w_n^p) for a listed party p, zero for an absent one
};
// one batch inversion: prefix products, the inverse of the last, and back
template <class P>
inline GaoInvLambda<Fp<P>> gao_make_inv_lambda(const GaoAbsent<Fp<P>>& a) {
  using F = Fp<P>;
  GaoInvLambda<F> t;
  F pre[GAO_MAX_N];
  F acc = F::one();
  for (int p = 0; p < GAO_MAX_N; p++) {
    t.v[p] = F::zero(), pre[p] = acc;
    if ((a.listed >> p) & 1) acc = acc * a.ld.lam[p];
  }
  F inv = acc.inverse();
  for (int p = GAO_MAX_N - 1; p >= 0; p--)
    if ((a.listed >> p) & 1) t.v[p] = inv * pre[p], inv = inv * a.ld.lam[p];
  return t;
}
// put(p, row of party p, h(w_n^p)) for every listed party p named in the errpos of a corrected chunk: gao_repair_word for a
// result gao_absent_finish has passed.  row, ilam: lane p's row of the share matrix and 1 / Lambda(w_n^p); ilam(p) is read
// only by a lane that stores.
template <class F, class G, class Row, class ILam, class Put>
ZK_HD void gao_repair_word_parties(const G& g, const GaoResult<F, G, true>& r, Row row, ILam ilam, Put put) {
  gao_repair_word<F, G>(g, r, [&](int p, const F& v) { put(p, row(p), v * ilam(p)); });
}

// ---------------------------------------------------------------- a batch of words (zk_pss_repair_batch)
// Item i is a share matrix [n][nchunks] at shares + i * item_stride.  The items share ONE list of dirty chunks: an entry names
// (item, chunk) as item * nchunks + chunk in 32 bits -- also the index of the chunk in status and errpos [nitems][nchunks].
constexpr int GAO_BATCH_MAX = 48;      // KING_BATCH (pss.hpp): the items of one king launch
// the refusal: every entry fits 32 bits
ZK_HD bool gao_batch_fits(uint64_t nitems, uint64_t nchunks) {
  return nitems >= 1 && nitems <= (uint64_t)GAO_BATCH_MAX && nchunks < ((uint64_t)1 << 32) &&
         nitems * nchunks < ((uint64_t)1 << 32);
}
ZK_HD uint32_t gao_batch_entry(uint32_t item, uint32_t chunk, uint32_t nchunks) { return item * nchunks + chunk; }
ZK_HD void gao_batch_decode(uint32_t entry, uint32_t nchunks, uint32_t& item, uint32_t& chunk) {
  item = entry / nchunks;
  chunk = entry - item * nchunks;
}
// With a party list (zk_pss_repair_batch_parties) an item is the compact matrix [nparties][nchunks], row r the shares of
// parties[r]; the list, and so the two tables of zk_pss_repair_parties (GaoAbsent, GaoInvLambda), are the same for every item.

// ---------------------------------------------------------------- one call
// What every form has in common and where the forms differ; gao_run<FrP, REPAIR> (gao_impl.hpp) takes one.  REPAIR is the
// driver's template flag: false -- the unpack, `shares` read, secrets / message written; true -- the repair, `shares` written
// in place, secrets and message unused.
struct GaoCall {
  void* shares = nullptr;              // device: per item a matrix [np][nchunks], rows pitch() elements apart
  const uint32_t* ids = nullptr;       // host: np ascending party ids below n; null: 0 .. np - 1
  int np = 0;                          // np == n: all parties, no list
  int nitems = 1;                      // a batch: nitems matrices item_stride elements apart, ONE list of dirty chunks;
  size_t item_stride = 0;              //   status / errpos [nitems][nchunks], summary [nitems][3 + n].  A single word: 1 and 0
  size_t nchunks = 0;                  // chunks of an item; with a range its valid columns, range->cnt
  const GaoRange* range = nullptr;     // the word lies in a block with padding (king_range.hpp); a repair of one word only
  int dimension = 0;
  void* secrets = nullptr;             // [nchunks][l] or null
  void* message = nullptr;             // [dimension][nchunks] or null
  uint8_t* status = nullptr;           // [nitems][nchunks]; with a range [range->len], written at range->chunk(column)
  uint32_t* errpos = nullptr;          // as status, or null
  uint64_t* summary = nullptr;         // [nitems][3 + n] or null
  size_t pitch() const { return range ? range->stride : nchunks; }
  bool batch() const { return item_stride != 0; }
};

// A refusal: the return code and the text of zk_last_error; code ZK_OK: none.
struct GaoRefusal {
  int code;
  const char* msg;
};
// THE check of a party list: a valid count, ascending ids below n -- written to ids[GAO_MAX_N], 0 .. np - 1 for a null list --
// a dimension in 1 .. n - 1 and more shares than the dimension (pss.rs:183-186), refused in this order.  ids_only: stop
// behind the ids -- the point-share entry points refuse a dimension and too few shares at a place and with a text of their own.
inline GaoRefusal gao_list_check(const uint32_t* parties, int np, int dimension, int n, uint32_t* ids, bool ids_only = false) {
  if (np <= 0 || np > n) return {ZK_ERR_BAD_INPUT, "bad party count"};
  for (int i = 0; i < np; i++) {
    ids[i] = parties ? parties[i] : (uint32_t)i;
    if (ids[i] >= (uint32_t)n || (i > 0 && ids[i] <= ids[i - 1])) return {ZK_ERR_BAD_INPUT, "party ids must be ascending and < n"};
  }
  if (ids_only) return {ZK_OK, nullptr};
  if (dimension < 1 || dimension > n - 1) return {ZK_ERR_BAD_INPUT, "dimension must lie in 1 .. n - 1"};
  if (np <= dimension) return {ZK_ERR_PROTOCOL, "Not enough shares to reconstruct"};
  return {ZK_OK, nullptr};
}
// Every refusal of a call, in the order the entry points have always tried them.  A call of no chunks is no refusal and
// its pointers are not looked at.  (What a batch adds -- the item count, the item stride -- is its entry point's:
// engine_gao.inc.hpp repair_batch_check.)
inline GaoRefusal gao_call_check(int l, const GaoCall& c, bool repair, uint32_t* ids) {
  if (const GaoRange* rg = c.range) {
    if (!repair || c.batch()) return {ZK_ERR_BAD_INPUT, "the range form is a repair of one word"};
    if (rg->cnt > rg->stride || rg->cnt > rg->len || rg->base >= (rg->len ? rg->len : 1) || rg->shift > rg->len ||
        rg->stride > 0xffffffffull || c.nchunks != rg->cnt)
      return {ZK_ERR_BAD_INPUT, "bad range: cnt <= stride < 2^32, cnt <= len, base < len, shift <= len"};
  }
  if (l != 1 && l != 2 && l != 4 && l != 8) return {ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8"};
  const GaoRefusal r = gao_list_check(c.ids, c.np, c.dimension, 4 * l, ids);
  if (r.code || c.nchunks == 0) return r;
  if (!c.shares || !c.status) return {ZK_ERR_BAD_INPUT, "null pointer"};
  if (c.nchunks >= ((uint64_t)1 << 32)) return {ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks"};
  return {ZK_OK, nullptr};
}

// ---------------------------------------------------------------- working memory of a call
// [0] the count of dirty chunks; from byte 32 the summary words of the items, (3 + n) each, used when the caller passes none;
// for a party list the table GaoAbsent and, for a repair, GaoInvLambda; then the ONE list of dirty chunks, room for every chunk
// of every item.  Byte offsets, multiples of 32: a call clears [0, tab); without tables tab == inv == list.  A caller may
// place this behind memory of its own (the checked h chain puts it behind its six vectors) and sizes it with `bytes`.
struct GaoLayout {
  size_t tab, inv, list, bytes;
};
ZK_HD GaoLayout gao_layout(int n, int nitems, size_t nchunks, size_t tab_size, size_t inv_size) {
  GaoLayout w;
  w.tab = (32 + (size_t)nitems * (3 + n) * 8 + 31) / 32 * 32;
  w.inv = w.tab + (tab_size + 31) / 32 * 32;
  w.list = w.inv + (inv_size + 31) / 32 * 32;
  w.bytes = w.list + (size_t)nitems * nchunks * 4;
  return w;
}
// with the tables' real sizes; list: the call has a party list (np < n), repair: it is one
template <class F>
ZK_HD GaoLayout gao_layout(int n, int nitems, size_t nchunks, bool list, bool repair = true) {
  return gao_layout(n, nitems, nchunks, list ? sizeof(GaoAbsent<F>) : 0, list && repair ? sizeof(GaoInvLambda<F>) : 0);
}
// The names the batch forms have for the same layout (their host tests, tests/native/gao_batch*_host_test.cpp, use them):
// the head of a batch without tables and its size, and the layout with the two tables of a party list.
using GaoBatchPartiesWork = GaoLayout;
ZK_HD size_t gao_batch_head(int n, int nitems) { return gao_layout(n, nitems, 0, 0, 0).list; }
ZK_HD size_t gao_batch_work_bytes(int n, int nitems, size_t nchunks) { return gao_layout(n, nitems, nchunks, 0, 0).bytes; }
ZK_HD GaoLayout gao_batch_parties_work(int n, int nitems, size_t nchunks, size_t tab_size, size_t inv_size) {
  return gao_layout(n, nitems, nchunks, tab_size, inv_size);
}
template <class F>
ZK_HD GaoLayout gao_batch_parties_work(int n, int nitems, size_t nchunks) {
  return gao_layout<F>(n, nitems, nchunks, true);
}

#if defined(__HIPCC__)
class IEngine;
// The one host driver, instantiated per curve in gao_<curve>.hip: the refusals of gao_call_check, one clear of the head of
// wk (and of the caller's summary), with a party list the launches that put its tables into wk, stage 1 and stage 2 -- no
// host synchronisation.  wk: device memory of gao_layout<Fr>(4 l, nitems, nchunks, np < 4 l, REPAIR).bytes bytes that the
// caller holds; a refused call and one of no chunks do not touch it.  A range of no columns clears the summary.
template <class FrP, bool REPAIR>
int gao_run(IEngine* e, void* wk, int l, const GaoCall& call, hipStream_t st);
#endif

}  // namespace zk
