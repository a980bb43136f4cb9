// Membership in the order-r subgroups G1 and G2 of BN254 and BLS12-381: the endomorphism maps and the predicate.
//
// Replaces ark-ec's `SWCurveConfig::is_in_correct_subgroup_assuming_on_curve` as ark-bn254 and ark-bls12-381 0.4 override
// it, which `CanonicalDeserialize::deserialize_compressed` (Validate::Yes) calls after the curve equation.  The truth is
// "[r]P = O"; each group is tested through an endomorphism whose eigenvalue on the subgroup is a short multiple of the
// curve parameter x, so a test is one or two fixed chains of 63 / 64 doublings instead of the 254 / 255 of [r]P:
//
//   BN254 G1       cofactor 1: the curve equation decides.
//   BN254 G2       [x + 1]P + psi([x]P) + psi^2([x]P) = psi^3([2x]P)           (eprint 2022/352, section 4.3; equivalent
//                                                                               to ark-bn254's psi(P) = [6x^2]P)
//   BLS12-381 G2   psi(P) = [x]P = -[|x|]P                                     (ark-bls12-381; Scott, eprint 2021/1130)
//   BLS12-381 G1   phi(P) = -[x^2]P, phi(x, y) = (beta x, y)                   (ark-bls12-381; beta = BETA_G1^2 of
//                                                                               glv_params.hpp, whose own eigenvalue is x^2 - 1)
//
// psi = twist . Frobenius . untwist on E'(Fq2): psi(x, y) = (conj(x) gx, conj(y) gy), gx = XI^((q-1)/3), gy = XI^((q-1)/2) on
// a D-type twist (FROB[0][2], FROB[0][3] of pairing_params.hpp) and their inverses on an M-type twist (subgroup_params.hpp).
//
// Plain single-lane host + device code like ec.hpp and tower.hpp: tests/native/subgroup_host_test.cpp compiles it for the
// host.  The chains run over compile-time constants; no loop bound depends on point data, and the only data-dependent
// branches are the forward ones of the group law (identity, equal inputs).
#pragma once
#include "ec.hpp"
#include "glv_params.hpp"
#include "subgroup_params.hpp"
#include "tower.hpp"

namespace zk {

template <class Fld>
ZK_HD_NOINLINE XYZZ<Fld> xyzz_madd_ni(const XYZZ<Fld>& a, const Fld& x2, const Fld& y2) {
  return xyzz_madd(a, x2, y2);
}

template <class F>
ZK_HD bool coord_is_canonical(const F& a) {
  if constexpr (IsExtField<F>::value) return a.c0.is_canonical() && a.c1.is_canonical();
  else return a.is_canonical();
}

template <class PP>
struct Subgroup {
  using T = Tower<PP>;
  using SP = SubgroupParams<PP>;
  using Fq = typename T::Fq;
  using F2 = typename T::F2;
  static constexpr bool BN = PP::BN_FROB_LINES;        // BN254; otherwise BLS12-381
  static constexpr uint64_t X = SP::X;                 // |x|
  static constexpr int X_BITS = 64 - __builtin_clzll(SP::X);

  static ZK_HD F2 psi_cx() {
    if constexpr (PP::TWIST_D) return T::template frob_coeff<1, 2>();
    else return T::f2_const(SP::PSI_X);
  }
  static ZK_HD F2 psi_cy() {
    if constexpr (PP::TWIST_D) return T::template frob_coeff<1, 3>();
    else return T::f2_const(SP::PSI_Y);
  }
  // psi of an affine point of the twist ((0,0) stays (0,0))
  static ZK_HD Affine<F2> psi(const Affine<F2>& p) { return {T::conj2(p.x) * psi_cx(), T::conj2(p.y) * psi_cy()}; }
  // ... and of a projective one: x = X / ZZ, y = Y / ZZZ, so the denominators are conjugated only
  static ZK_HD XYZZ<F2> psi(const XYZZ<F2>& p) {
    return {T::conj2(p.X) * psi_cx(), T::conj2(p.Y) * psi_cy(), T::conj2(p.ZZ), T::conj2(p.ZZZ)};
  }
  // phi(x, y) = (beta x, y) on G1 of BLS12-381, beta the cube root of unity with phi = -[x^2] on the subgroup
  static ZK_HD Fq beta() {
    static_assert(!BN, "G1 of BN254 has cofactor 1");
    const Fq b = Fq::from_limbs(Glv<Bls381Fr>::BETA_G1);
    return Fq::mul_ni(b, b);
  }
  static ZK_HD Affine<Fq> phi(const Affine<Fq>& p) { return {Fq::mul_ni(p.x, beta()), p.y}; }

  // [|x|] p by a fixed double-and-add chain over the bits of the constant; p affine and not the identity
  template <class Fld>
  static ZK_HD XYZZ<Fld> mul_x(const Affine<Fld>& p) {
    XYZZ<Fld> r = XYZZ<Fld>::from_affine(p);
#pragma unroll 1
    for (int b = X_BITS - 2; b >= 0; b--) {
      r = xyzz_dbl_ni(r);
      if ((X >> b) & 1) r = xyzz_madd_ni(r, p.x, p.y);
    }
    return r;
  }
  template <class Fld>
  static ZK_HD XYZZ<Fld> mul_x(const XYZZ<Fld>& p) {
    XYZZ<Fld> r = p;
#pragma unroll 1
    for (int b = X_BITS - 2; b >= 0; b--) {
      r = xyzz_dbl_ni(r);
      if ((X >> b) & 1) r = xyzz_add_ni(r, p);
    }
    return r;
  }
  // a = b as points
  template <class Fld>
  static ZK_HD bool same(const XYZZ<Fld>& a, const XYZZ<Fld>& b) {
    if (a.is_identity() || b.is_identity()) return a.is_identity() && b.is_identity();
    return a.X * b.ZZ == b.X * a.ZZ && a.Y * b.ZZZ == b.Y * a.ZZZ;
  }
  // (x, y) = -b
  template <class Fld>
  static ZK_HD bool is_neg_of(const Affine<Fld>& p, const XYZZ<Fld>& b) {
    if (b.is_identity()) return false;
    return p.x * b.ZZ == b.X && p.y * b.ZZZ == b.Y.neg();
  }

  // on the curve, not the identity -> in the order-r subgroup
  static ZK_HD bool g1_in_subgroup(const Affine<Fq>& p) {
    if constexpr (BN) return true;
    else return is_neg_of(phi(p), mul_x(mul_x(p)));
  }
  static ZK_HD bool g2_in_subgroup(const Affine<F2>& p) {
    if constexpr (BN) {
      const XYZZ<F2> xp = mul_x(p);
      const XYZZ<F2> p1 = psi(xp), p2 = psi(p1), p3 = psi(p2);
      const XYZZ<F2> lhs = xyzz_add_ni(xyzz_add_ni(xyzz_madd_ni(xp, p.x, p.y), p1), p2);
      return same(lhs, xyzz_dbl_ni(p3));
    } else {
      return is_neg_of(psi(p), mul_x(p));
    }
  }

  template <class Fld>
  static ZK_HD bool on_curve(const Affine<Fld>& p, const Fld& b) {
    return p.y.sqr() == p.x.sqr() * p.x + b;
  }
  static ZK_HD F2 twist_b() { return T::f2_const(PP::TWIST_B); }

  // the whole predicate over affine Montgomery limbs as they cross the ABI: both coordinates below q, and the identity
  // (0, 0) or a point of the curve with [r]P = O
  static ZK_HD bool g1_check(const Affine<Fq>& p, int b1) {
    if (!coord_is_canonical(p.x) || !coord_is_canonical(p.y)) return false;
    if (p.is_identity()) return true;
    if (!on_curve(p, Fq::from_u64((uint64_t)b1))) return false;
    return g1_in_subgroup(p);
  }
  static ZK_HD bool g2_check(const Affine<F2>& p) {
    if (!coord_is_canonical(p.x) || !coord_is_canonical(p.y)) return false;
    if (p.is_identity()) return true;
    if (!on_curve(p, twist_b())) return false;
    return g2_in_subgroup(p);
  }
};

}  // namespace zk
