// Host build of the subgroup membership tests (csrc/subgroup.hpp).  Reads one case per line from stdin:
//   <curve: bn254 | bls12_381> <op> <hex integers>
// ops: g1 x y | g2 x0 x1 y0 y1 -> the verdict of g1_check / g2_check, 0 or 1;
//      psi x0 x1 y0 y1 -> the four coordinates of psi(P);  phi x y -> the two of phi(P) (BLS12-381 only).
// Coordinates cross as the limbs the ABI carries (Montgomery form, read as plain integers), unconverted, so that values
// of q and above reach the predicate as they are.  tests/test_native_subgroup.py compares with Python integers.
#include <cstdio>
#include <cstring>
#include <string>

#include "subgroup.hpp"

using namespace zk;

template <class Fq>
static Fq parse(const char* hex) {
  Fq r = Fq::zero();
  const size_t n = strlen(hex);
  for (size_t i = 0; i < n; i++) {
    const char c = hex[n - 1 - i];
    const uint32_t d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    if (i / 8 < (size_t)Fq::N) r.v[i / 8] |= d << (4 * (i % 8));
  }
  return r;
}
template <class Fq>
static void print(const Fq& c) {
  bool lead = true;
  for (int i = Fq::N - 1; i >= 0; i--) {
    if (lead && c.v[i] == 0 && i > 0) continue;
    printf(lead ? "%x" : "%08x", c.v[i]);
    lead = false;
  }
}

template <class PP, int B1>
static int run(const std::string& op, char tok[4][128]) {
  using S = Subgroup<PP>;
  using Fq = typename S::Fq;
  using F2 = typename S::F2;
  if (op == "g1") {
    printf("%d\n", (int)S::g1_check(Affine<Fq>{parse<Fq>(tok[0]), parse<Fq>(tok[1])}, B1));
  } else if (op == "g2" || op == "psi") {
    const Affine<F2> p{F2{parse<Fq>(tok[0]), parse<Fq>(tok[1])}, F2{parse<Fq>(tok[2]), parse<Fq>(tok[3])}};
    if (op == "g2") {
      printf("%d\n", (int)S::g2_check(p));
    } else {
      const Affine<F2> r = S::psi(p);
      const Fq* c[4] = {&r.x.c0, &r.x.c1, &r.y.c0, &r.y.c1};
      for (int i = 0; i < 4; i++) print(*c[i]), putchar(i == 3 ? '\n' : ' ');
    }
  } else if (op == "phi") {
    if constexpr (S::BN) return 1;
    else {
      const Affine<Fq> r = S::phi(Affine<Fq>{parse<Fq>(tok[0]), parse<Fq>(tok[1])});
      print(r.x), putchar(' '), print(r.y), putchar('\n');
    }
  } else {
    return 1;
  }
  return 0;
}

int main() {
  char curve[32], op[32];
  static char tok[4][128];
  while (scanf("%31s %31s", curve, op) == 2) {
    const int n = (!strcmp(op, "g1") || !strcmp(op, "phi")) ? 2 : 4;
    for (int i = 0; i < n; i++)
      if (scanf("%127s", tok[i]) != 1) return 2;
    int rc;
    if (!strcmp(curve, "bn254")) rc = run<PairingBn254, 3>(op, tok);
    else if (!strcmp(curve, "bls12_381")) rc = run<PairingBls381, 4>(op, tok);
    else rc = 1;
    if (rc) return rc;
  }
  return 0;
}
