// Host-side run of the repair form of csrc/gao.hpp with a party list (zk_pss_repair_parties): the table of the list
// (gao_make_absent) and the inverses 1 / Lambda(w^p) (gao_make_inv_lambda, one batch inversion); the scan as its SP lanes run
// it -- the load that multiplies by Lambda(w^p), the clean test at dimension k + rho, no secrets, no message -- and for a dirty
// word the decoder over GaoHostGroup with its flag RE at k + rho, gao_absent_finish on that result (errpos masked against the
// list, a phantom demoted) and gao_repair_word_parties, which writes h'(w^p) / Lambda(w^p) into the party's row: the program
// text the kernels compile.
//   gao_repair_parties_host_test <f17|bn254> <l>      reads one case per line from stdin:
//       k np id_0 ... id_{np-1} y_0 ... y_{np-1}       (ascending party ids; the shares of the listed, canonical hex)
//   and prints per case:  status errpos y'_0 ... y'_{np-1}      (the listed shares after the repair)
// f17: the field of gao.rs's own tests, l <= 4 (its largest subgroup has 16 elements).
// Built and run by tests/test_native_gao_repair_parties.py with the host compiler, once more under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "curves.hpp"
#include "gao.hpp"
using namespace zk;

// F17 on two 32-bit limbs: R = 2^64 = 1 mod 17, so Montgomery form is the integer itself; generator 3, which has order 16
struct F17P {
  static constexpr int N = 2;
  static constexpr int BITS = 5;
  static constexpr uint32_t N0INV = 0x0f0f0f0fu;
  static constexpr uint32_t MOD[2] = {17u, 0u};
  static constexpr uint32_t R1[2] = {1u, 0u};
  static constexpr uint32_t R2[2] = {1u, 0u};
  static constexpr int TWO_ADICITY = 4;
  static constexpr uint32_t GENERATOR[2] = {3u, 0u};
  static constexpr uint32_t TWO_ADIC_ROOT[2] = {3u, 0u};
};

template <class F> F parse(const std::string& hex) {
  F r = F::zero();
  size_t n = hex.size();
  for (size_t i = 0; i < n; i++) {
    char c = hex[n - 1 - i];
    uint32_t d = c >= 'a' ? c - 'a' + 10 : c >= 'A' ? c - 'A' + 10 : c - '0';
    if (i / 8 < (size_t)F::N) r.v[i / 8] |= d << (4 * (i % 8));
  }
  return r.to_mont();
}
template <class F> void print(const F& x) {
  F c = x.from_mont();
  printf(" ");
  for (int i = F::N - 1; i >= 0; i--) printf("%08x", c.v[i]);
}

template <class F, int L> int run() {
  constexpr int N = 4 * L;
  using G = GaoHostGroup;
  using VF = G::V<F>;
  const GaoConsts<F> c = gao_make_consts<typename F::Params>(L);
  const G g{N};
  const VF xp = g.make<F>([&](int p) { return gao_lane_pow<F, 5>(c.wpow2, p); });
  const VF xinv = g.make<F>([&](int p) { return gao_lane_pow<F, 5>(c.wipow2, p); });
  const VF sp = g.make<F>([&](int) { return F::zero(); });      // the repair form evaluates no secrets
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    int k, np;
    if (!(is >> k >> np)) continue;
    if (k < 1 || np <= k || np > N) return 2;
    uint32_t ids[N];
    for (int i = 0; i < np; i++) {
      if (!(is >> ids[i]) || ids[i] >= (uint32_t)N || (i && ids[i] <= ids[i - 1])) return 2;
    }
    std::vector<F> word(np);
    for (int i = 0; i < np; i++) {
      std::string t;
      if (!(is >> t)) return 2;
      word[i] = parse<F>(t);
    }
    const GaoAbsent<F> a = gao_make_absent<typename F::Params>(c, L, ids, np, k);
    const GaoInvLambda<F> il = gao_make_inv_lambda<typename F::Params>(a);
    const int kd = k + a.rho;
    auto ld = [&](int p) { return a.ld.row[p] < 0 ? F::zero() : word[a.ld.row[p]] * a.ld.lam[p]; };
    int status = 0;
    uint32_t errpos = 0;
    // the scan as its SP lanes run it, one after the other
    constexpr int SP = gao_split(L), M = N / SP;
    F x[SP][M];
    bool clean = true;
    for (int q = 0; q < SP; q++) {
      gao_load<M, SP>(c, q, ld, x[q]);
      gao_ifft<M, SP>(c, x[q]);
      clean = gao_is_clean<M, SP>(x[q], kd, q) && clean;
    }
    if (!clean) {
      const VF y = g.make<F>(ld);
      GaoResult<F, G, true> r = gao_chunk<F, G, true>(g, c, N, kd, true, y, xp, xinv, sp);
      gao_absent_finish<F, G, true>(g, k, a.rho, a.listed, false, sp, sp, r);      // (no secrets, no message: slam, lamc unread)
      status = r.status;
      errpos = r.errpos;
      gao_repair_word_parties<F, G>(
          g, r, [&](int p) { return a.ld.row[p]; }, [&](int p) { return il.v[p]; },
          [&](int, int row, const F& v) { word.at(row) = v; });
    }
    printf("%d %x", status, errpos);
    for (int i = 0; i < np; i++) print(word[i]);
    printf("\n");
  }
  return 0;
}
template <class P> int by_l(int l, int max_l) {
  using F = Fp<P>;
  if (l > max_l) return 2;
  switch (l) {
    case 1: return run<F, 1>();
    case 2: return run<F, 2>();
    case 4: return run<F, 4>();
    case 8:
      if constexpr (P::TWO_ADICITY >= 5) return run<F, 8>();
  }
  return 2;
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int l = atoi(argv[2]);
  if (!strcmp(argv[1], "f17")) return by_l<F17P>(l, 4);
  if (!strcmp(argv[1], "bn254")) return by_l<Bn254Fr>(l, 8);
  return 2;
}
