// Host-side run of csrc/gao.hpp, the error-correcting unpack of zk_pss_unpack_robust: the one-lane syndrome test and clean
// unpack of stage 1, and for a dirty word the decoder of stage 2 over GaoHostGroup (an array of n lanes in place of the wave's
// cross-lane builtins) -- the program text the kernels compile.
//   gao_host_test <bn254|bls381|bls377> <l>      reads one case per line from stdin:  k y_0 ... y_{n-1}
// (canonical integers, hex) and prints per case:  status errpos h_0 ... h_{k-1} s_0 ... s_{l-1}
// Built and run by tests/test_native_gao.py with the host compiler, once more under ASan + UBSan.
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
  const VF sp = g.make<F>([&](int p) { return c.g * gao_lane_pow<F, 3>(c.spow2, p & 7); });
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    int k;
    if (!(is >> k)) continue;
    if (k < 1 || k > N - 1) return 2;
    VF y{};
    for (int p = 0; p < N; p++) {
      std::string t;
      if (!(is >> t)) return 2;
      y.a[p] = parse<F>(t);
    }
    std::vector<F> h(k, F::zero());
    F sec[L];
    for (int i = 0; i < L; i++) sec[i] = F::zero();
    int status = 0;
    uint32_t errpos = 0;
    // stage 1 as its SP lanes run it, one after the other
    constexpr int SP = gao_split(L), M = N / SP;
    F x[SP][M];
    bool clean = true;
    for (int q = 0; q < SP; q++) {
      gao_load<M, SP>(c, q, [&](int p) { return y.a[p]; }, x[q]);
      gao_ifft<M, SP>(c, x[q]);
      clean = gao_is_clean<M, SP>(x[q], k, q) && clean;
    }
    if (clean) {
      for (int q = 0; q < SP; q++) {
        gao_clean_secrets<M, SP>(c, x[q], k, q, [&](int i, const F& v) { sec[i] = sec[i] + v; });
        gao_clean_message<M, SP>(c, x[q], k, q, [&](int j, const F& v) { h[j] = v; });
      }
    } else {
      GaoResult<F, G> r = gao_chunk<F, G>(g, c, N, k, true, y, xp, xinv, sp);
      status = r.status;
      errpos = r.errpos;
      for (int j = 0; j < k; j++) h[j] = r.h.a[j];
      for (int i = 0; i < L; i++) sec[i] = r.sec.a[i];
    }
    printf("%d %x", status, errpos);
    for (int j = 0; j < k; j++) print(h[j]);
    for (int i = 0; i < L; i++) print(sec[i]);
    printf("\n");
  }
  return 0;
}
template <class P> int by_l(int l) {
  using F = Fp<P>;
  switch (l) {
    case 1: return run<F, 1>();
    case 2: return run<F, 2>();
    case 4: return run<F, 4>();
    case 8: return run<F, 8>();
  }
  return 2;
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int l = atoi(argv[2]);
  if (!strcmp(argv[1], "bn254")) return by_l<Bn254Fr>(l);
  if (!strcmp(argv[1], "bls381")) return by_l<Bls381Fr>(l);
  if (!strcmp(argv[1], "bls377")) return by_l<Bls377Fr>(l);
  return 2;
}
