// Host-side check of the row map of the batched checked h chain (csrc/h_batch.hpp staging_row): the three repairs of a batch
// write a round-major staging report and h_report_gather_kernel reads row staging_row(nb, b, k) for row 7 b + k of the
// proof-major report.  For every batch size 1 .. 16:
//   * staging_row is a bijection from (proof, item) onto 0 .. 7 nb - 1,
//   * the rows of a round are contiguous, start at staging_round_first and come in the item order of that round's repair
//     (item 3 b + k of rounds 0 and 1, item b of the deg_red round) -- the order gao_impl.hpp's batch kernels index by,
//   * walked as the gather kernel walks it over real buffers, every report row receives the bytes of its own (proof, item).
// Prints one line per violation, then "batches B rows R", then "V violations".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "h_batch.hpp"

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
  size_t batches = 0, rows = 0;
  for (uint32_t nb = 1; nb <= (uint32_t)H_BATCH_MAX; nb++) {
    batches++;
    const uint32_t total = H_REPORT_ROWS * nb;
    std::vector<uint32_t> hits(total, 0);
    for (uint32_t b = 0; b < nb; b++)
      for (uint32_t k = 0; k < (uint32_t)H_REPORT_ROWS; k++) {
        const uint32_t r = staging_row(nb, b, k);
        CHECK(r < total, "nb %u: proof %u item %u maps to row %u of %u", nb, b, k, r, total);
        if (r < total) hits[r]++;
        const uint32_t round = k / 3, item = round < 2 ? 3 * b + k % 3 : b;
        CHECK(r == staging_round_first(nb, round) + item, "nb %u: proof %u item %u is row %u, not item %u of round %u", nb, b, k,
              r, item, round);
        CHECK(item < staging_round_items(nb, round), "nb %u: item %u of round %u is beyond the round", nb, item, round);
      }
    for (uint32_t r = 0; r < total; r++) CHECK(hits[r] == 1, "nb %u: row %u hit %u times", nb, r, hits[r]);
    // the rounds tile 0 .. 7 nb - 1 in order, and a round is what one repair call takes
    uint32_t end = 0;
    for (uint32_t round = 0; round < 3; round++) {
      CHECK(staging_round_first(nb, round) == end, "nb %u: round %u starts at %u, not %u", nb, round, staging_round_first(nb, round), end);
      CHECK(staging_round_items(nb, round) <= (uint32_t)H_BATCH_ITEMS, "nb %u: round %u has %u items", nb, round, staging_round_items(nb, round));
      end += staging_round_items(nb, round);
    }
    CHECK(end == total, "nb %u: the rounds end at %u of %u", nb, end, total);
    // the gather, on the host: staging row s holds the byte pattern of its (round, item); report row 7 b + k must end up
    // with the pattern of proof b, item k
    const uint32_t nchunks = 5;
    std::vector<uint8_t> staging((size_t)total * nchunks), report((size_t)total * nchunks, 0xff);
    for (uint32_t round = 0; round < 3; round++)
      for (uint32_t item = 0; item < staging_round_items(nb, round); item++) {
        const uint32_t b = round < 2 ? item / 3 : item, k = round < 2 ? 3 * round + item % 3 : 6;
        for (uint32_t c = 0; c < nchunks; c++)
          staging[(size_t)(staging_round_first(nb, round) + item) * nchunks + c] = (uint8_t)(b * 8 + k);
      }
    for (uint32_t row = 0; row < total; row++) {
      const size_t src = staging_row(nb, row / H_REPORT_ROWS, row % H_REPORT_ROWS);
      for (uint32_t c = 0; c < nchunks; c++) report[(size_t)row * nchunks + c] = staging[src * nchunks + c];
    }
    for (uint32_t b = 0; b < nb; b++)
      for (uint32_t k = 0; k < (uint32_t)H_REPORT_ROWS; k++)
        for (uint32_t c = 0; c < nchunks; c++)
          CHECK(report[((size_t)b * H_REPORT_ROWS + k) * nchunks + c] == (uint8_t)(b * 8 + k), "nb %u: report row of proof %u item %u holds %u", nb,
                b, k, report[((size_t)b * H_REPORT_ROWS + k) * nchunks + c]);
    rows += total;
  }
  std::printf("batches %zu rows %zu\n", batches, rows);
  std::printf("%d violations\n", bad);
  return bad != 0;
}
