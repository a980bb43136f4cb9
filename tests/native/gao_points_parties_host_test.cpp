// Host-side run of the party-list forms of csrc/gao_points.hpp (zk_pss_repair_points_parties,
// zk_pss_unpack_points_robust_parties) over BN254 G1: the table gao_points_make_list builds for a (list, dimension), the rows of
// stage 1 -- gao_points_row with the table's syndrome coefficients over the compact shares -- and for a dirty word the
// lane-group decoder gao_points_chunk_parties over GaoHostGroup: the program text the kernels compile.
//   gao_points_parties_host_test <l>      reads one request per line from stdin
//     L s                                            -> x y      the point s G (G = (1, 2)), affine; "0 0" for the identity
//     W k np id_0 .. id_{np-1} y_0 .. y_{np-1}       -> status errpos x_0 y_0 ... x_{np-1} y_{np-1}
//                                                       the compact word (y_i G: the share of party id_i) after the repair
//     U k np id_0 .. id_{np-1} y_0 .. y_{np-1}       -> status errpos x_0 y_0 ... x_{l-1} y_{l-1}
//                                                       the unpack form: the l secrets of the clean or corrected word (the
//                                                       identity for a failed one) through the table's Lagrange matrix
// (canonical integers, hex).  Built and run by tests/test_native_gao_points_parties.py with the host compiler, once more under
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
    int k, np;
    if ((what != "W" && what != "U") || !(is >> k >> np) || k < 1 || k > n - 1 || np <= k || np > n) return 2;
    uint32_t ids[GAO_MAX_N];
    for (int i = 0; i < np; i++)
      if (!(is >> ids[i]) || ids[i] >= (uint32_t)n || (i && ids[i] <= ids[i - 1])) return 2;
    A y[GAO_MAX_N];
    for (int i = 0; i < np; i++) {
      if (!(is >> t)) return 2;
      y[i] = gao_pt_to_affine(gao_pt_mul<Bn254Fr, Fq>(gen, parse<Fr>(t)));
    }
    const GaoPtListHost<Fr> host = gao_points_make_list<Bn254Fr>(l, ids, np, k);
    const GaoPtList<Fr> lt = host.view();
    // stage 1: the syndrome rows, one after the other
    const int nsyn = np - k;
    A syn[GAO_MAX_N];
    bool clean = true;
    for (int i = 0; i < nsyn; i++) {
      const XYZZ<Fq> s = gao_points_row<Bn254Fr, Fq>(
          np, [&](int c) { return lt.syn + (size_t)i * np + c; }, [&](int c) { return y[c]; });
      if (!s.is_identity()) clean = false;
      syn[i] = gao_pt_to_affine(s);
    }
    const auto synf = [&](int i) { return syn[i]; };
    int status = 0;
    uint32_t errpos = 0;
    if (what == "U") {
      A out[8];
      for (int i = 0; i < l; i++)
        out[i] = gao_pt_to_affine(gao_points_row<Bn254Fr, Fq>(
            np, [&](int c) { return lt.umat + (size_t)i * np + c; }, [&](int c) { return y[c]; }));
      if (!clean) {
        const GaoPtResult<Fq, G> r = gao_points_chunk_parties<Bn254Fr, Fq, G, false>(
            g, &tab, lt, n, l, true, synf, [&](int, int i) { return out[i]; },
            [&](int i, int q) { return lt.umat[(size_t)i * np + lt.row[q]]; });
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
      const GaoPtResult<Fq, G> r = gao_points_chunk_parties<Bn254Fr, Fq, G, true>(
          g, &tab, lt, n, 1, true, synf, [&](int q, int) { return y[lt.row[q]]; }, [&](int, int) { return Fr::zero(); });
      status = r.status;
      errpos = r.errpos;
      if (status == 1) y[lt.row[gao_top_bit(errpos)]] = r.val.a[0];
    }
    printf("%d %x", status, errpos);
    for (int i = 0; i < np; i++) print(y[i]);
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
