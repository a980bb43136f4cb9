// Host-side run of csrc/gao_points.hpp (zk_pss_repair_points, zk_pss_unpack_points_robust) over BN254 G1: the rows of stage 1 -- gao_points_row with the
// syndrome coefficients -- and for a dirty word the lane-group decoder gao_points_chunk over GaoHostGroup with its flag RE,
// whose output replaces the share errpos names: the program text the kernels compile.
//   gao_points_host_test <l>      reads one request per line from stdin
//     L s                      -> x y                              the point s G (G = (1, 2)), affine; "0 0" for the identity
//     W k y_0 ... y_{n-1}      -> status errpos x_0 y_0 ... x_{n-1} y_{n-1}      the word (y_p G) after the repair
//     U k y_0 ... y_{n-1}      -> status errpos x_0 y_0 ... x_{l-1} y_{l-1}      the unpack form: the l secrets of the clean or
//                                 corrected word (the identity for a failed one), through stage 1's secret rows and the
//                                 decoder without RE -- the products U[i][q] w^(q k) S_k
// (canonical integers, hex).  Built and run by tests/test_native_gao_points.py with the host compiler, once more under
// ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "curves.hpp"
#include "gao_points.hpp"
using namespace zk;

using Fr = Fp<Bn254Fr>;
using Fq = Fp<Bn254Fq>;
using A = Affine<Fq>;

template <class F> F parse(const std::string& hex) {
  F r = F::zero();
  size_t n = hex.size();
  for (size_t i = 0; i < n; i++) {
    char c = hex[n - 1 - i];
    uint32_t d = c >= 'a' ? c - 'a' + 10 : c >= 'A' ? c - 'A' + 10 : c - '0';
    if (i / 8 < (size_t)F::N) r.v[i / 8] |= d << (4 * (i % 8));
  }
  return r;                       // canonical
}
void print(const Fq& x) {
  Fq c = x.from_mont();
  printf(" ");
  for (int i = Fq::N - 1; i >= 0; i--) printf("%08x", c.v[i]);
}
void print(const A& a) {
  print(a.x);
  print(a.y);
}

int run(int l) {
  const int n = 4 * l;
  using G = GaoHostGroup;
  const G g{n};
  const GaoPtTable<Fr> tab = gao_points_make_table<Bn254Fr>(l);
  const GaoConsts<Fr> c = gao_make_consts<Bn254Fr>(l);
  const A gen{Fq::one(), Fq::from_u64(2)};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string what, t;
    if (!(is >> what)) continue;
    if (what == "L") {
      if (!(is >> t)) return 2;
      print(gao_pt_to_affine(gao_pt_mul<Bn254Fr, Fq>(gen, parse<Fr>(t))));
      printf("\n");
      continue;
    }
    int k;
    if ((what != "W" && what != "U") || !(is >> k) || k < 1 || k > n - 1) return 2;
    A y[GAO_MAX_N];
    for (int p = 0; p < n; p++) {
      if (!(is >> t)) return 2;
      y[p] = gao_pt_to_affine(gao_pt_mul<Bn254Fr, Fq>(gen, parse<Fr>(t)));
    }
    // stage 1: the syndrome rows, one after the other
    A syn[GAO_MAX_N];
    bool clean = true;
    for (int i = 0; i < n - k; i++) {
      const XYZZ<Fq> s = gao_points_row<Bn254Fr, Fq>(
          n, [&](int p) { return gao_points_syn_coef(&tab, n, k, i, p); }, [&](int p) { return y[p]; });
      if (!s.is_identity()) clean = false;
      syn[i] = gao_pt_to_affine(s);
    }
    int status = 0;
    uint32_t errpos = 0;
    if (what == "U") {
      // the unpack matrix as the engine builds it: U[i][p] = 1/n sum_{d < D} (s_i / x_p)^d, D = 2l up to dimension 2l, else n
      Fr um[8 * GAO_MAX_N];
      const int D = k <= 2 * l ? 2 * l : n;
      for (int i = 0; i < l; i++)
        for (int p = 0; p < n; p++) {
          const Fr ratio = c.sec[i] * gao_lane_pow<Fr, 5>(c.wipow2, p);
          Fr acc = Fr::zero(), cur = Fr::one();
          for (int d = 0; d < D; d++) acc = acc + cur, cur = cur * ratio;
          um[i * n + p] = (acc * c.ninv).from_mont();
        }
      A out[8];
      for (int i = 0; i < l; i++)
        out[i] = gao_pt_to_affine(gao_points_row<Bn254Fr, Fq>(
            n, [&](int p) { return &um[i * n + p]; }, [&](int p) { return y[p]; }));
      if (!clean) {
        const GaoPtResult<Fq, G> r = gao_points_chunk<Bn254Fr, Fq, G, false>(
            g, &tab, n, k, l, true, [&](int i) { return syn[i]; }, [&](int, int i) { return out[i]; },
            [&](int i, int q) { return um[i * n + q]; });
        status = r.status;
        errpos = r.errpos;
        for (int i = 0; i < l; i++) out[i] = r.val.a[i];
      }
      printf("%d %x", status, errpos);
      for (int i = 0; i < l; i++) print(out[i]);
      printf("\n");
      continue;
    }
    if (!clean) {
      const GaoPtResult<Fq, G> r = gao_points_chunk<Bn254Fr, Fq, G, true>(
          g, &tab, n, k, 1, true, [&](int i) { return syn[i]; }, [&](int q, int) { return y[q]; },
          [&](int, int) { return Fr::zero(); });
      status = r.status;
      errpos = r.errpos;
      if (status == 1) y[gao_top_bit(errpos)] = r.val.a[0];
    }
    printf("%d %x", status, errpos);
    for (int p = 0; p < n; p++) print(y[p]);
    printf("\n");
  }
  return 0;
}
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int l = atoi(argv[1]);
  if (l != 1 && l != 2 && l != 4) return 2;
  return run(l);
}
