// Host build of the single-lane Fq12 tower (csrc/tower.hpp).  Reads one case per line from stdin:
//   <curve: bn254 | bls12_381> <op> <24 hex integers: a (12, memory order), b (12)>
// and prints the 12 coefficients of the result as hex integers.  Values cross as canonical integers; the Montgomery
// conversion happens here.  ops: mul sqr inv conj frob1 frob2 frob3 cyc line (line: b's first six integers are
// l0, lS, l3 of the sparse element l0 + lS w^S + l3 w^3).  tests/test_native_tower.py compares with Python integers.
#include <cstdio>
#include <cstring>
#include <string>

#include "tower.hpp"

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
  return r.to_mont();
}
template <class Fq>
static void print(const Fq& x) {
  const Fq c = x.from_mont();
  bool lead = true;
  for (int i = Fq::N - 1; i >= 0; i--) {
    if (lead && c.v[i] == 0 && i > 0) continue;
    printf(lead ? "%x" : "%08x", c.v[i]);
    lead = false;
  }
}

template <class PP>
static int run(const std::string& op, char tok[24][128]) {
  using T = Tower<PP>;
  using Fq = typename T::Fq;
  using F2 = typename T::F2;
  typename T::Fq12 a, b, r;
  Fq* pa = reinterpret_cast<Fq*>(&a);
  Fq* pb = reinterpret_cast<Fq*>(&b);
  static_assert(sizeof(a) == 12 * sizeof(Fq), "Fq12 is twelve packed Fq");
  for (int i = 0; i < 12; i++) pa[i] = parse<Fq>(tok[i]), pb[i] = parse<Fq>(tok[12 + i]);
  if (op == "mul") r = T::mul(a, b);
  else if (op == "sqr") r = T::sqr(a);
  else if (op == "inv") r = T::inverse(a);
  else if (op == "conj") r = T::conj(a);
  else if (op == "frob1") r = T::template frobenius<1>(a);
  else if (op == "frob2") r = T::template frobenius<2>(a);
  else if (op == "frob3") r = T::template frobenius<3>(a);
  else if (op == "cyc") r = T::cyclotomic_sqr(a);
  else if (op == "line") r = T::mul_by_line(a, F2{pb[0], pb[1]}, F2{pb[2], pb[3]}, F2{pb[4], pb[5]});
  else return 1;
  const Fq* pr = reinterpret_cast<const Fq*>(&r);
  for (int i = 0; i < 12; i++) {
    print(pr[i]);
    putchar(i == 11 ? '\n' : ' ');
  }
  return 0;
}

int main() {
  char curve[32], op[32];
  static char tok[24][128];
  while (scanf("%31s %31s", curve, op) == 2) {
    for (int i = 0; i < 24; i++)
      if (scanf("%127s", tok[i]) != 1) return 2;
    int rc;
    if (!strcmp(curve, "bn254")) rc = run<PairingBn254>(op, tok);
    else if (!strcmp(curve, "bls12_381")) rc = run<PairingBls381>(op, tok);
    else rc = 1;
    if (rc) return rc;
  }
  return 0;
}
