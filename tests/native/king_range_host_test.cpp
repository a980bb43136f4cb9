// Host-side check of the chunk ranges of the all-to-all king and of the column -> chunk map of a rank's block
// (csrc/king_range.hpp king_span / king_chunk / GaoRange): for every word length, number of present ranks, granule and shift
// the ranges of all present ranks must hit every chunk 0 .. len - 1 exactly once, no column >= cnt may be mapped, and the
// ranges must be the ones a2a_pack_kernel fills (pss.hpp: column c of present rank i holds chunk (i * seg + c - shift) mod len
// while i * seg + c < len).
// Prints one line per violation, then "cases C applicable A chunks N", then "V violations".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "king_range.hpp"

using namespace zk;

static int bad = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      bad++;                                  \
      std::printf("violation: " __VA_ARGS__); \
      std::printf("\n");                      \
    }                                         \
  } while (0)

int main() {
  size_t cases = 0, applicable = 0, chunks = 0;
  for (uint32_t len = 8; len <= 8192; len *= 2)
    for (uint32_t ranks = 2; ranks <= 8; ranks++)
      for (int big = 0; big < 2; big++)
        for (uint32_t shift = 0; shift < 2; shift++) {
          const uint32_t gran = big ? (len < 256 ? len : 256) : 1;
          cases++;
          std::vector<uint32_t> hits(len, 0);
          bool ok = true, any = false;
          uint32_t seg0 = 0, end = 0;
          for (uint32_t me = 0; me < ranks; me++) {
            KingSpan sp{0, 0, 0};
            const bool r = king_span(len, gran, ranks, me, &sp);
            CHECK(me == 0 || r == ok, "len %u ranks %u gran %u: rank %u disagrees on whether the plan applies", len, ranks, gran, me);
            ok = r;
            if (!r) continue;
            any = true;
            if (me == 0) seg0 = sp.seg;
            CHECK(sp.seg == seg0 && sp.seg % gran == 0 && sp.seg > 0, "len %u ranks %u gran %u rank %u: seg %u", len, ranks, gran, me, sp.seg);
            CHECK(sp.cnt <= sp.seg && sp.cnt % gran == 0, "len %u ranks %u gran %u rank %u: cnt %u of seg %u", len, ranks, gran, me, sp.cnt, sp.seg);
            CHECK(sp.rs == end && (uint64_t)sp.rs + sp.cnt <= len, "len %u ranks %u gran %u rank %u: rs %u cnt %u after %u", len, ranks, gran, me, sp.rs, sp.cnt, end);
            CHECK(sp.cnt == 0 || sp.rs == me * sp.seg, "len %u ranks %u gran %u rank %u: rs %u is not me * seg", len, ranks, gran, me, sp.rs);
            end = sp.rs + sp.cnt;
            // the block as the repair sees it: stride seg, cnt valid columns, base rs
            const GaoRange rg{sp.seg, sp.cnt, sp.cnt ? sp.rs : 0u, shift, len};
            for (uint32_t c = 0; c < sp.seg; c++) {
              const bool filled = (uint64_t)me * sp.seg + c < len;      // a2a_pack_kernel writes this column
              CHECK(filled == (c < sp.cnt), "len %u ranks %u gran %u rank %u: column %u filled %d, cnt %u", len, ranks, gran, me, c, (int)filled, sp.cnt);
              if (c >= sp.cnt) continue;                                 // columns >= cnt are never mapped
              const uint32_t j = rg.chunk(c);
              CHECK(j < len, "len %u ranks %u gran %u rank %u: column %u maps to %u", len, ranks, gran, me, c, j);
              CHECK(j == (uint32_t)(((uint64_t)me * sp.seg + c + len - shift) % len), "len %u ranks %u gran %u rank %u: column %u maps to %u, the pack holds another chunk", len, ranks, gran, me, c, j);
              CHECK(gao_range_dev(rg).chunk(c) == j, "len %u ranks %u gran %u rank %u: the kernels' form maps column %u to %u, not %u", len, ranks, gran, me, c, gao_range_dev(rg).chunk(c), j);
              if (j < len) hits[j]++;
            }
          }
          CHECK(any == (len / gran >= ranks), "len %u ranks %u gran %u: applies %d", len, ranks, gran, (int)any);
          if (!any) continue;
          applicable++;
          CHECK(end == len, "len %u ranks %u gran %u: the ranges end at %u", len, ranks, gran, end);
          for (uint32_t j = 0; j < len; j++)
            CHECK(hits[j] == 1, "len %u ranks %u gran %u shift %u: chunk %u hit %u times", len, ranks, gran, shift, j, hits[j]);
          chunks += len;
        }
  // the whole word is the range with stride == cnt == len, base 0, shift 0: the identity map
  for (uint32_t len = 1; len <= 4096; len = len * 3 + 1) {
    const GaoRange whole{len, len, 0, 0, len};
    for (uint32_t c = 0; c < len; c++)
      CHECK(whole.chunk(c) == c && gao_range_dev(whole).chunk(c) == c, "whole word of %u: column %u maps to %u", len, c, whole.chunk(c));
  }
  // refusals: no granule per rank, a length that is no multiple of the granule, one rank, a rank index out of range
  KingSpan sp;
  CHECK(!king_span(4, 1, 5, 0, &sp) && !king_span(12, 8, 2, 0, &sp) && !king_span(64, 1, 1, 0, &sp) && !king_span(64, 1, 4, 4, &sp) &&
            !king_span(64, 0, 4, 0, &sp),
        "a plan that must not apply did");
  std::printf("cases %zu applicable %zu chunks %zu\n", cases, applicable, chunks);
  std::printf("%d violations\n", bad);
  return bad != 0;
}
