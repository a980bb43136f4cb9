// Host build of the shared text of zk_pss_repair_batch (csrc/gao.hpp): the packing of a dirty-list entry, its decode, the
// refusal predicate and the layout of the working memory.  Reads lines from stdin and answers each on stdout:
//   e <nitems> <nchunks> <item> <chunk>   ->  <entry> <decoded item> <decoded chunk>
//   f <nitems> <nchunks>                  ->  <gao_batch_fits: 0 or 1>
//   w <n> <nitems> <nchunks>              ->  gao_layout without tables: <list, the end of the head> <bytes>
// tests/test_native_gao_batch.py writes the cases and checks the answers against Python integers.
#include <cinttypes>
#include <cstdio>

#include "gao.hpp"

int main() {
  char op;
  while (std::scanf(" %c", &op) == 1) {
    if (op == 'e') {
      uint64_t nitems, nchunks, item, chunk;
      if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &nitems, &nchunks, &item, &chunk) != 4) return 2;
      if (!zk::gao_batch_fits(nitems, nchunks) || item >= nitems || chunk >= nchunks) return 3;      // the driver's precondition
      const uint32_t entry = zk::gao_batch_entry((uint32_t)item, (uint32_t)chunk, (uint32_t)nchunks);
      uint32_t di = ~0u, dc = ~0u;
      zk::gao_batch_decode(entry, (uint32_t)nchunks, di, dc);
      std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", entry, di, dc);
    } else if (op == 'f') {
      uint64_t nitems, nchunks;
      if (std::scanf("%" SCNu64 " %" SCNu64, &nitems, &nchunks) != 2) return 2;
      std::printf("%d\n", zk::gao_batch_fits(nitems, nchunks) ? 1 : 0);
    } else if (op == 'w') {
      int n, nitems;
      uint64_t nchunks;
      if (std::scanf("%d %d %" SCNu64, &n, &nitems, &nchunks) != 3) return 2;
      const zk::GaoLayout w = zk::gao_layout(n, nitems, (size_t)nchunks, 0, 0);
      std::printf("%zu %zu\n", w.list, w.bytes);
    } else {
      return 2;
    }
  }
  return 0;
}
