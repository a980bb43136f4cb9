// Host-side run of zk_pss_repair_batch_parties' shared text (csrc/gao.hpp): a batch of items, each a compact matrix
// [np][nchunks] of ONE party list, through what the two kernels of the call compile -- laid out in working memory by
// gao_layout (the head of a batch, the two tables of the list, the one dirty list):
//   scan    per (item, chunk), as its SP lanes run it: the load whose row is the popcount of the `listed` mask below the
//           party and which multiplies by Lambda(w^p), the clean test at dimension k + rho; a dirty chunk is appended to the
//           one list as gao_batch_entry(item, chunk)
//   repair  per list entry (walked from the back: the entries of a walk belong to any items in any order):
//           gao_batch_decode, the load through the table in working memory, the decoder over GaoHostGroup with its flag RE,
//           gao_absent_finish, gao_repair_word_parties into the item's matrix, the per-chunk adds to the item's summary words
//   gao_batch_parties_host_test <f17|bn254> <l>      reads batches from stdin until it ends:
//       k np id_0 ... id_{np-1} nitems nchunks pad                      (one line)
//       y_0 ... y_{np-1}                                                (nitems * nchunks lines, item by item; canonical hex)
//   and prints per batch: per (item, chunk) a line  status errpos y'_0 ... y'_{np-1},  per item a line with its 3 + n summary
//   words, and one line  tab inv list bytes sizeof(GaoAbsent) sizeof(GaoInvLambda) pad_ok.
//   gao_batch_parties_host_test layout                reads lines  n nitems nchunks tab_size inv_size  and prints the four
//   offsets of gao_layout for each.
// Built and run by tests/test_native_gao_batch_parties.py with the host compiler, once more under ASan + UBSan.
#include <cinttypes>
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
  using Tab = GaoAbsent<F>;
  using Inv = GaoInvLambda<F>;
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
    if (k < 1 || np <= k || np >= N) return 2;                   // (np == n is zk_pss_repair_batch itself)
    uint32_t ids[N];
    for (int i = 0; i < np; i++)
      if (!(is >> ids[i]) || ids[i] >= (uint32_t)N || (i && ids[i] <= ids[i - 1])) return 2;
    uint64_t nitems, nchunks, pad;
    if (!(is >> nitems >> nchunks >> pad)) return 2;
    if (!gao_batch_fits(nitems, nchunks) || !nchunks) return 3;   // the driver's precondition
    const size_t per = (size_t)np * nchunks, stride = per + pad;
    const F sentinel = parse<F>("b");
    std::vector<F> shares(stride * nitems, sentinel);
    for (uint64_t it = 0; it < nitems; it++)
      for (uint64_t ch = 0; ch < nchunks; ch++) {
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream ws(line);
        for (int r = 0; r < np; r++) {
          std::string t;
          if (!(ws >> t)) return 2;
          shares[it * stride + (size_t)r * nchunks + ch] = parse<F>(t);
        }
      }
    // ---- working memory, as the driver lays it out: everything below is read and written THROUGH it
    const GaoLayout lay = gao_layout<F>(N, (int)nitems, (size_t)nchunks, true);
    std::vector<unsigned char> work(lay.bytes, 0xEE);
    std::memset(work.data(), 0, lay.tab);                          // the one clear: the count and the items' summary words
    uint32_t count = 0;
    auto summary = [&](uint32_t item, int word) { return work.data() + 32 + ((size_t)item * (3 + N) + word) * 8; };
    auto sum_add = [&](uint32_t item, int word) {
      unsigned long long v;
      std::memcpy(&v, summary(item, word), 8);
      v++;
      std::memcpy(summary(item, word), &v, 8);
    };
    {
      const Tab a = gao_make_absent<typename F::Params>(c, L, ids, np, k);
      const Inv il = gao_make_inv_lambda<typename F::Params>(a);
      std::memcpy(work.data() + lay.tab, &a, sizeof(Tab));
      std::memcpy(work.data() + lay.inv, &il, sizeof(Inv));
    }
    Tab tab;
    Inv inv;
    std::memcpy(&tab, work.data() + lay.tab, sizeof(Tab));
    std::memcpy(&inv, work.data() + lay.inv, sizeof(Inv));
    const int rho = tab.rho, kd = k + rho;
    const uint32_t listed = tab.listed;
    std::vector<int> status(nitems * nchunks, -1);
    std::vector<uint32_t> errpos(nitems * nchunks, ~0u);
    // ---- the scan: item on the outer axis, the row of party p from the mask
    constexpr int SP = gao_split(L), M = N / SP;
    for (uint32_t it = 0; it < nitems; it++) {
      const F* sh = shares.data() + it * stride;
      const uint32_t entry0 = gao_batch_entry(it, 0, (uint32_t)nchunks);
      for (uint32_t j = 0; j < nchunks; j++) {
        auto ld = [&](int p) {
          const int row = __builtin_popcount(listed & ((1u << p) - 1));
          return (listed >> p) & 1 ? sh[(size_t)row * nchunks + j] * tab.ld.lam[p] : F::zero();
        };
        F x[SP][M];
        bool clean = true;
        for (int q = 0; q < SP; q++) {
          gao_load<M, SP>(c, q, ld, x[q]);
          gao_ifft<M, SP>(c, x[q]);
          clean = gao_is_clean<M, SP>(x[q], kd, q) && clean;
        }
        if (clean) {
          status[entry0 + j] = 0, errpos[entry0 + j] = 0;
          sum_add(it, 0);
        } else {
          const uint32_t e = entry0 + j;
          std::memcpy(work.data() + lay.list + 4 * (size_t)count++, &e, 4);
        }
      }
    }
    // ---- the repair: one walk over the one list, from the back
    for (uint32_t gi = count; gi-- > 0;) {
      uint32_t entry, item, chunk;
      std::memcpy(&entry, work.data() + lay.list + 4 * (size_t)gi, 4);
      gao_batch_decode(entry, (uint32_t)nchunks, item, chunk);
      if (item >= nitems || chunk >= nchunks) return 4;
      F* sh = shares.data() + item * stride;
      const VF y = g.make<F>([&](int p) {
        const int row = tab.ld.row[p];
        return row >= 0 ? sh[(size_t)row * nchunks + chunk] * tab.ld.lam[p] : F::zero();
      });
      GaoResult<F, G, true> r = gao_chunk<F, G, true>(g, c, N, kd, true, y, xp, xinv, sp);
      gao_absent_finish<F, G, true>(g, k, rho, listed, false, sp, sp, r);      // (no secrets, no message: slam, lamc unread)
      gao_repair_word_parties<F, G>(
          g, r, [&](int p) { return tab.ld.row[p]; }, [&](int p) { return inv.v[p]; },
          [&](int, int row, const F& v) { sh[(size_t)row * nchunks + chunk] = v; });
      status[entry] = r.status, errpos[entry] = r.errpos;
      sum_add(item, r.status == 1 ? 1 : 2);
      for (int p = 0; p < N; p++)
        if ((r.errpos >> p) & 1) sum_add(item, 3 + p);
    }
    bool pad_ok = true;
    for (uint64_t it = 0; it < nitems; it++) {
      for (uint64_t ch = 0; ch < nchunks; ch++) {
        printf("%d %x", status[it * nchunks + ch], errpos[it * nchunks + ch]);
        for (int r = 0; r < np; r++) print(shares[it * stride + (size_t)r * nchunks + ch]);
        printf("\n");
      }
      for (size_t i = per; i < stride; i++) pad_ok = pad_ok && shares[it * stride + i] == sentinel;
    }
    for (uint32_t it = 0; it < nitems; it++) {
      for (int w = 0; w < 3 + N; w++) {
        unsigned long long v;
        std::memcpy(&v, summary(it, w), 8);
        printf("%s%llu", w ? " " : "", v);
      }
      printf("\n");
    }
    printf("%zu %zu %zu %zu %zu %zu %d\n", lay.tab, lay.inv, lay.list, lay.bytes, sizeof(Tab), sizeof(Inv), pad_ok ? 1 : 0);
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
int layout() {
  int n, nitems;
  uint64_t nchunks, tab, inv;
  while (std::scanf("%d %d %" SCNu64 " %" SCNu64 " %" SCNu64, &n, &nitems, &nchunks, &tab, &inv) == 5) {
    const GaoLayout w = gao_layout(n, nitems, (size_t)nchunks, (size_t)tab, (size_t)inv);
    std::printf("%zu %zu %zu %zu\n", w.tab, w.inv, w.list, w.bytes);
  }
  return 0;
}
int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc != 3) return 2;
  const int l = atoi(argv[2]);
  if (!strcmp(argv[1], "f17")) return by_l<F17P>(l, 4);
  if (!strcmp(argv[1], "bn254")) return by_l<Bn254Fr>(l, 8);
  return 2;
}
