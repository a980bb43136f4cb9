// Host-side run of csrc/setup.hpp's quotient vectors (the Lagrange coefficients at tau and h_query in closed form, with the
// lane-local batch inversion over a run of consecutive indices), as quotient_kernel's lanes run them on the device.
//   setup_host_test <bn254|bls381> <lagrange|h> <len> <run> <hex field elements ...>
// lagrange takes tau, k, root, root_inv; h takes tau, tau_n, k, root, root_inv, start (canonical integers, big-endian hex).
// One lane per run of `run` indices (the last run is short when `run` does not divide `len`); prints out[0 .. len) as
// canonical hex integers, one per line.  Built and run by tests/test_native_setup.py with the host compiler.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "curves.hpp"
#include "setup.hpp"
using namespace zk;

template <class F> F parse(const char* hex) {
  F r = F::zero();
  size_t n = strlen(hex);
  for (size_t i = 0; i < n; i++) {
    char c = hex[n - 1 - i];
    uint32_t d = c >= 'a' ? c - 'a' + 10 : c >= 'A' ? c - 'A' + 10 : c - '0';
    if (i / 8 < (size_t)F::N) r.v[i / 8] |= d << (4 * (i % 8));
  }
  return r.to_mont();
}
template <class F> void print(const F& x) {
  F c = x.from_mont();
  for (int i = F::N - 1; i >= 0; i--) printf("%08x", c.v[i]);
  printf("\n");
}
template <class F, class Term> void lanes(const Term& t, size_t len, size_t run) {
  std::vector<F> out(len);
  for (size_t begin = 0; begin < len; begin += run) quotient_run<F, Term>(t, begin, len - begin < run ? len - begin : run, out.data());
  for (const F& x : out) print(x);
}
template <class P> int run(int argc, char** argv) {
  using F = Fp<P>;
  const bool h = !strcmp(argv[2], "h");
  const size_t len = strtoull(argv[3], nullptr, 10), rn = strtoull(argv[4], nullptr, 10);
  if (argc != 5 + (h ? 6 : 4) || !len || !rn) return 2;
  F a[6];
  for (int i = 0; i < argc - 5; i++) a[i] = parse<F>(argv[5 + i]);
  if (h) lanes<F>(HTerm<F>{a[0], a[1], a[2], a[3], a[4], a[5]}, len, rn);
  else lanes<F>(LagrangeTerm<F>{a[0], a[1], a[2], a[3]}, len, rn);
  return 0;
}
int main(int argc, char** argv) {
  if (argc < 6) return 2;
  if (!strcmp(argv[1], "bn254")) return run<Bn254Fr>(argc, argv);
  if (!strcmp(argv[1], "bls381")) return run<Bls381Fr>(argc, argv);
  return 2;
}
