// The Fq12 tower of the pairing: Fq6 = Fq2[v]/(v^3 - XI), Fq12 = Fq6[w]/(w^2 - v) over Fp2T (field.hpp).
//
// Replaces, on the verifier's path, ark-ff's Fp6 / Fp12 (`QuadExtField<Fp12ConfigWrapper>`: mul, square, inverse,
// frobenius_map, cyclotomic_square, mul_by_034 / mul_by_014) reached from ark-ec's `Pairing::multi_pairing`.
//
// Two forms of the same arithmetic:
//  * Tower<PP>: plain single-lane host + device code on the nested struct Fq12 = (c0, c1) over Fq6 = (b0, b1, b2) over
//    Fq2 -- the memory order of arkworks' Fp12 and of snarkjs' [2][3][2] nesting.  It is what the host test compiles and
//    what the lane-split form is checked against; on the device only the one inversion of a final exponentiation runs it.
//  * Lane12<PP> (device): one Fq12 value split over a group of GW = 8 lanes.  Fq12 = Fq2[w]/(w^6 - XI) with the basis
//    1, w, ..., w^5 (w^j sits in c_{j mod 2}.b_{j div 2}); lane j < 6 of the group holds the Fq2 coefficient of w^j, lanes
//    6 and 7 mirror lanes 0 and 1 and never store.  A product is c_j = sum_i a_i b_{(j - i) mod 6} (times XI when i > j):
//    six Fq2 products per lane with the operands fetched by ds_bpermute (__shfl), control flow uniform in the group as in
//    quad.hpp.  A lane then holds a handful of Fq2 values (16 / 24 dwords each) instead of 96 / 144 dwords per Fq12 value.
#pragma once
#include "field.hpp"
#include "pairing_params.hpp"

namespace zk {

template <class PP>
struct Tower {
  using Fq = Fp<typename PP::FqP>;
  using F2 = Fp2<typename PP::FqP>;
  static constexpr int N = Fq::N;
  struct Fq6 {
    F2 b0, b1, b2;
  };
  struct Fq12 {
    Fq6 c0, c1;
  };

  static ZK_HD F2 f2_const(const uint32_t (&c)[2][N]) { return {Fq::from_limbs(c[0]), Fq::from_limbs(c[1])}; }
  static ZK_HD F2 conj2(const F2& a) { return {a.c0, a.c1.neg()}; }
  static ZK_HD F2 scale2(const F2& a, const Fq& k) { return {Fq::mul_ni(a.c0, k), Fq::mul_ni(a.c1, k)}; }
  // a * (XI0 + u), XI0 = 1 or 9
  static ZK_HD F2 mul_xi(const F2& a) {
    static_assert(PP::XI1 == 1 && (PP::XI0 == 1 || PP::XI0 == 9), "non-residue");
    if constexpr (PP::XI0 == 1) return {a.c0 - a.c1, a.c1 + a.c0};
    else {
      const Fq t0 = a.c0.dbl().dbl().dbl() + a.c0, t1 = a.c1.dbl().dbl().dbl() + a.c1;
      return {t0 - a.c1, t1 + a.c0};
    }
  }
  template <int K, int J>
  static ZK_HD F2 frob_coeff() {
    return f2_const(PP::FROB[K - 1][J]);
  }

  // ---- Fq6
  static ZK_HD Fq6 zero6() { return {F2::zero(), F2::zero(), F2::zero()}; }
  static ZK_HD Fq6 add6(const Fq6& a, const Fq6& b) { return {a.b0 + b.b0, a.b1 + b.b1, a.b2 + b.b2}; }
  static ZK_HD Fq6 sub6(const Fq6& a, const Fq6& b) { return {a.b0 - b.b0, a.b1 - b.b1, a.b2 - b.b2}; }
  static ZK_HD Fq6 neg6(const Fq6& a) { return {a.b0.neg(), a.b1.neg(), a.b2.neg()}; }
  static ZK_HD Fq6 mulv(const Fq6& a) { return {mul_xi(a.b2), a.b0, a.b1}; }
  // Karatsuba over Fq2: 6 products
  static ZK_HD_NOINLINE Fq6 mul6(const Fq6& a, const Fq6& b) {
    const F2 v0 = a.b0 * b.b0, v1 = a.b1 * b.b1, v2 = a.b2 * b.b2;
    const F2 c0 = v0 + mul_xi((a.b1 + a.b2) * (b.b1 + b.b2) - v1 - v2);
    const F2 c1 = (a.b0 + a.b1) * (b.b0 + b.b1) - v0 - v1 + mul_xi(v2);
    const F2 c2 = (a.b0 + a.b2) * (b.b0 + b.b2) - v0 - v2 + v1;
    return {c0, c1, c2};
  }
  static ZK_HD Fq6 scale6(const Fq6& a, const F2& k) { return {a.b0 * k, a.b1 * k, a.b2 * k}; }
  static ZK_HD Fq6 inv6(const Fq6& a) {
    const F2 t0 = a.b0.sqr() - mul_xi(a.b1 * a.b2);
    const F2 t1 = mul_xi(a.b2.sqr()) - a.b0 * a.b1;
    const F2 t2 = a.b1.sqr() - a.b0 * a.b2;
    const F2 d = a.b0 * t0 + mul_xi(a.b2 * t1 + a.b1 * t2);
    return scale6({t0, t1, t2}, d.inverse_fast());
  }

  // ---- Fq12
  static ZK_HD Fq12 one() { return {{F2::one(), F2::zero(), F2::zero()}, zero6()}; }
  static ZK_HD bool eq(const Fq12& a, const Fq12& b) {
    return a.c0.b0 == b.c0.b0 && a.c0.b1 == b.c0.b1 && a.c0.b2 == b.c0.b2 && a.c1.b0 == b.c1.b0 && a.c1.b1 == b.c1.b1 &&
           a.c1.b2 == b.c1.b2;
  }
  // coefficient of w^j
  static ZK_HD F2& coef(Fq12& a, int j) {
    Fq6& h = (j & 1) ? a.c1 : a.c0;
    return (j >> 1) == 0 ? h.b0 : (j >> 1) == 1 ? h.b1 : h.b2;
  }
  static ZK_HD const F2& coef(const Fq12& a, int j) {
    const Fq6& h = (j & 1) ? a.c1 : a.c0;
    return (j >> 1) == 0 ? h.b0 : (j >> 1) == 1 ? h.b1 : h.b2;
  }
  static ZK_HD Fq12 mul(const Fq12& a, const Fq12& b) {
    const Fq6 t0 = mul6(a.c0, b.c0), t1 = mul6(a.c1, b.c1);
    return {add6(t0, mulv(t1)), sub6(sub6(mul6(add6(a.c0, a.c1), add6(b.c0, b.c1)), t0), t1)};
  }
  // complex squaring: c0 = (a0 + a1)(a0 + v a1) - t - v t, c1 = 2 t, t = a0 a1
  static ZK_HD Fq12 sqr(const Fq12& a) {
    const Fq6 t = mul6(a.c0, a.c1);
    const Fq6 s = mul6(add6(a.c0, a.c1), add6(a.c0, mulv(a.c1)));
    return {sub6(sub6(s, t), mulv(t)), add6(t, t)};
  }
  static ZK_HD Fq12 conj(const Fq12& a) { return {a.c0, neg6(a.c1)}; }
  static ZK_HD Fq12 inverse(const Fq12& a) {
    const Fq6 d = inv6(sub6(mul6(a.c0, a.c0), mulv(mul6(a.c1, a.c1))));
    return {mul6(a.c0, d), neg6(mul6(a.c1, d))};
  }
  // a^(q^K): the coefficient of w^j becomes conj^K(a_j) * XI^(j (q^K - 1) / 6)
  template <int K>
  static ZK_HD Fq12 frobenius(const Fq12& a) {
    auto cj = [](const F2& x) { return (K & 1) ? conj2(x) : x; };
    Fq12 r;
    r.c0.b0 = cj(a.c0.b0);
    r.c1.b0 = cj(a.c1.b0) * frob_coeff<K, 1>();
    r.c0.b1 = cj(a.c0.b1) * frob_coeff<K, 2>();
    r.c1.b1 = cj(a.c1.b1) * frob_coeff<K, 3>();
    r.c0.b2 = cj(a.c0.b2) * frob_coeff<K, 4>();
    r.c1.b2 = cj(a.c1.b2) * frob_coeff<K, 5>();
    return r;
  }
  // (x + y s)^2 in Fq4 = Fq2[s]/(s^2 - XI)
  static ZK_HD void sqr4(const F2& x, const F2& y, F2* t0, F2* t1) {
    const F2 xx = x.sqr(), yy = y.sqr();
    *t0 = mul_xi(yy) + xx;
    *t1 = (x + y).sqr() - xx - yy;
  }
  // Granger-Scott squaring of an element of the cyclotomic subgroup (anything raised to (q^6 - 1)(q^2 + 1)): three Fq4
  // squarings over the pairs (a_0, a_3), (a_1, a_4), (a_2, a_5) of w-basis coefficients
  static ZK_HD Fq12 cyclotomic_sqr(const Fq12& a) {
    F2 t0, t1, t2, t3, t4, t5;
    sqr4(coef(a, 0), coef(a, 3), &t0, &t1);
    sqr4(coef(a, 1), coef(a, 4), &t2, &t3);
    sqr4(coef(a, 2), coef(a, 5), &t4, &t5);
    const F2 x5 = mul_xi(t5);
    Fq12 r;
    coef(r, 0) = (t0 - coef(a, 0)).dbl() + t0;
    coef(r, 1) = (x5 + coef(a, 1)).dbl() + x5;
    coef(r, 2) = (t2 - coef(a, 2)).dbl() + t2;
    coef(r, 3) = (t1 + coef(a, 3)).dbl() + t1;
    coef(r, 4) = (t4 - coef(a, 4)).dbl() + t4;
    coef(r, 5) = (t3 + coef(a, 5)).dbl() + t3;
    return r;
  }
  // a * (l0 + ls w^S + l3 w^3): the line of a Miller step.  S = 1 on a D-type twist (arkworks' mul_by_034), 2 on an
  // M-type twist (mul_by_014).
  static constexpr int LINE_S = PP::TWIST_D ? 1 : 2;
  static ZK_HD Fq12 mul_by_line(const Fq12& a, const F2& l0, const F2& ls, const F2& l3) {
    Fq12 r;
    for (int j = 0; j < 6; j++) {
      F2 lo = coef(a, j) * l0, hi = F2::zero();
      const int ks = j - LINE_S, k3 = j - 3;
      if (ks < 0) hi = hi + coef(a, ks + 6) * ls;
      else lo = lo + coef(a, ks) * ls;
      if (k3 < 0) hi = hi + coef(a, k3 + 6) * l3;
      else lo = lo + coef(a, k3) * l3;
      coef(r, j) = lo + mul_xi(hi);
    }
    return r;
  }
};

#if defined(__HIPCC__)
// ---- the lane-split form
constexpr int PAIRING_GW = 8;               // lanes of a group; 64 / GW groups per wave

template <class PP>
struct Lane12 {
  using T = Tower<PP>;
  using Fq = typename T::Fq;
  using F2 = typename T::F2;
  static constexpr int N = Fq::N;
  int j;        // the coefficient this lane holds (lanes 6, 7 of a group: 0, 1)
  int base;     // first lane of the group within the wave
  bool stores;  // lanes 0..5

  ZK_D static Lane12 here() {
    const int lane = (int)(threadIdx.x & 63u), g = lane & (PAIRING_GW - 1);
    return {g % 6, lane - g, g < 6};
  }
  // slot of w^j in the memory order c0.b0, c0.b1, c0.b2, c1.b0, c1.b1, c1.b2
  ZK_D int slot() const { return (j & 1) * 3 + (j >> 1); }
  // x as held by coefficient lane `src` of this group
  ZK_D F2 get(const F2& x, int src) const {
    F2 r;
    const int l = base + src;
#pragma unroll
    for (int i = 0; i < N; i++) {
      r.c0.v[i] = (uint32_t)__shfl((int)x.c0.v[i], l);
      r.c1.v[i] = (uint32_t)__shfl((int)x.c1.v[i], l);
    }
    return r;
  }
  ZK_D static F2 sel(bool c, const F2& a, const F2& b) {
    F2 r;
#pragma unroll
    for (int i = 0; i < N; i++) {
      r.c0.v[i] = c ? a.c0.v[i] : b.c0.v[i];
      r.c1.v[i] = c ? a.c1.v[i] : b.c1.v[i];
    }
    return r;
  }
  ZK_D F2 one() const { return sel(j == 0, F2::one(), F2::zero()); }
  ZK_D F2 load(const F2* p /* one Fq12 value */) const { return p[slot()]; }
  ZK_D void store(F2* p, const F2& a) const {
    if (stores) p[slot()] = a;
  }
  // every lane's copy of the whole value (for the single-lane inversion)
  ZK_D typename T::Fq12 gather(const F2& a) const {
    typename T::Fq12 r;
    T::coef(r, 0) = get(a, 0);
    T::coef(r, 1) = get(a, 1);
    T::coef(r, 2) = get(a, 2);
    T::coef(r, 3) = get(a, 3);
    T::coef(r, 4) = get(a, 4);
    T::coef(r, 5) = get(a, 5);
    return r;
  }
  ZK_D F2 pick(const typename T::Fq12& a) const {
    F2 r = T::coef(a, 0);
#pragma unroll
    for (int k = 1; k < 6; k++) r = sel(j == k, T::coef(a, k), r);
    return r;
  }

  ZK_D F2 mul(const F2& a, const F2& b) const {
    F2 lo = F2::zero(), hi = F2::zero();
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
      int k = j - i;
      const bool wrap = k < 0;
      k += wrap ? 6 : 0;
      const F2 t = get(a, i) * get(b, k);
      lo = sel(wrap, lo, lo + t);
      hi = sel(wrap, hi + t, hi);
    }
    return lo + T::mul_xi(hi);
  }
  ZK_D F2 sqr(const F2& a) const { return mul(a, a); }
  ZK_D F2 conj(const F2& a) const { return sel((j & 1) != 0, a.neg(), a); }
  template <int K>
  ZK_D F2 frobenius(const F2& a) const {
    F2 c = F2::one();
    c = sel(j == 1, T::template frob_coeff<K, 1>(), c);
    c = sel(j == 2, T::template frob_coeff<K, 2>(), c);
    c = sel(j == 3, T::template frob_coeff<K, 3>(), c);
    c = sel(j == 4, T::template frob_coeff<K, 4>(), c);
    c = sel(j == 5, T::template frob_coeff<K, 5>(), c);
    return ((K & 1) ? T::conj2(a) : a) * c;
  }
  ZK_D F2 inverse(const F2& a) const { return pick(T::inverse(gather(a))); }
  // Granger-Scott (Tower::cyclotomic_sqr): lanes j and j + 3 share one Fq4 squaring -- own^2 and own * partner per lane,
  // the partner's square by one exchange; then 3 t -+ 2 a_j with t taken from the lane that holds it
  ZK_D F2 cyclotomic_sqr(const F2& a) const {
    const int partner = j < 3 ? j + 3 : j - 3;
    const F2 p = get(a, partner);
    const F2 s = a.sqr(), m = a * p;
    const F2 ps = get(s, partner);
    const F2 t = sel(j < 3, s + T::mul_xi(ps), m.dbl());
    // lane j takes t from: 0 -> 0, 1 -> 5, 2 -> 1, 3 -> 3, 4 -> 2, 5 -> 4
    const int src = j == 0 ? 0 : j == 1 ? 5 : j == 2 ? 1 : j == 3 ? 3 : j == 4 ? 2 : 4;
    F2 tt = get(t, src);
    tt = sel(j == 1, T::mul_xi(tt), tt);
    const F2 d = sel((j & 1) != 0, tt + a, tt - a);
    return d.dbl() + tt;
  }
  // a * (l0 + ls w^S + l3 w^3); every lane of the group holds the same l0, ls, l3
  ZK_D F2 mul_by_line(const F2& a, const F2& l0, const F2& ls, const F2& l3) const {
    constexpr int S = T::LINE_S;
    const bool ws = j < S, w3 = j < 3;
    const F2 as = get(a, ws ? j - S + 6 : j - S), a3 = get(a, w3 ? j + 3 : j - 3);
    const F2 t0 = a * l0, ts = as * ls, t3 = a3 * l3;
    const F2 z = F2::zero();
    const F2 lo = t0 + sel(ws, z, ts) + sel(w3, z, t3);
    const F2 hi = sel(ws, ts, z) + sel(w3, t3, z);
    return lo + T::mul_xi(hi);
  }
};
#endif

}  // namespace zk
