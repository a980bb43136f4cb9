// Host-side run of the absent-party forms of csrc/gao.hpp (zk_pss_unpack_robust_parties): the table of a party list
// (gao_make_absent), stage 1 as its SP lanes run it -- the load that multiplies by Lambda(w^p), the clean test and the secrets
// at dimension k + rho, the message deflated root by root (gao_deflate, the two lanes of a split exchanging through a
// snapshot of each other) -- and for a dirty word stage 2 over GaoHostGroup with gao_absent_finish behind the decoder: the
// program text the kernels compile.
//   gao_erasure_host_test <bn254|bls381|bls377> <l>      reads one case per line from stdin:
//       k np id_0 ... id_{np-1} y_0 ... y_{np-1}          (ascending party ids; the shares of the listed, canonical hex)
//   and prints per case:  status errpos h_0 ... h_{k-1} s_0 ... s_{l-1}
// Built and run by tests/test_native_gao_erasure.py with the host compiler, once more under ASan + UBSan.
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
    const int kd = k + a.rho;
    auto ld = [&](int p) { return a.ld.row[p] < 0 ? F::zero() : word[a.ld.row[p]] * a.ld.lam[p]; };
    std::vector<F> h(k, F::zero());
    F sec[L];
    for (int i = 0; i < L; i++) sec[i] = F::zero();
    int status = 0;
    uint32_t errpos = 0;
    constexpr int SP = gao_split(L), M = N / SP;
    F x[SP][M];
    bool clean = true;
    for (int q = 0; q < SP; q++) {
      gao_load<M, SP>(c, q, ld, x[q]);
      gao_ifft<M, SP>(c, x[q]);
      clean = gao_is_clean<M, SP>(x[q], kd, q) && clean;
    }
    if (clean) {
      for (int q = 0; q < SP; q++)
        gao_clean_secrets<M, SP>(c, x[q], kd, q, [&](int i) { return a.sscale[i]; },
                                 [&](int i, const F& v) { sec[i] = sec[i] + v; });
      for (int e = 0; e < a.rho; e++) {
        F snap[SP][M];                  // what the lanes held before this root: the partner's sends come from here
        memcpy(snap, x, sizeof(x));
        for (int q = 0; q < SP; q++)
          gao_deflate<M, SP>(x[q], a.root[e], q, [&](int m, const F&) {
            if (q == 0) return snap[SP - 1][gao_bitrev(m, M)];                          // lane 1 sends its a at m
            return m + 1 < M ? snap[0][gao_bitrev(m + 1, M)] : F::zero();               // lane 0 its a at m + 1
          });
      }
      for (int q = 0; q < SP; q++)
        gao_clean_message<M, SP>(c, x[q], k, q, [&](int j, const F& v) { h[j] = v; });
    } else {
      const VF y = g.make<F>(ld);
      const VF slam = g.make<F>([&](int p) { return a.slam[p & 7]; });
      const VF lamc = g.make<F>([&](int p) { return a.lamc[p]; });
      GaoResult<F, G> r = gao_chunk<F, G>(g, c, N, kd, true, y, xp, xinv, sp);
      gao_absent_finish<F, G>(g, k, a.rho, a.listed, true, slam, lamc, r);
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
