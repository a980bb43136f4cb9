// Host-side check of the row map of the batched checked h chain (csrc/h_batch.hpp staging_row): the three repairs of a batch
// write a round-major staging report and h_report_gather_kernel reads row staging_row(nb, b, k) for row 7 b + k of the
// proof-major report.  For every batch size 1 .. 16:
//   * staging_row is a bijection from (proof, item) onto 0 .. 7 nb - 1,
//   * the rows of a round are contiguous, start at staging_round_first and come in the item order of that round's repair
//     (item 3 b + k of rounds 0 and 1, item b of the deg_red round) -- the order gao_impl.hpp's batch kernels index by,
//   * walked as the gather kernel walks it over real buffers, every report row receives the bytes of its own (proof, item).
// And of the layout of the chain's work buffer (h_layout), for every form of the chain: nb 1 .. 16, n in {4, 8, 16, 32} (l = n /
// 4), m/l in {1, 4, 512, 2^17}, unchecked / checked / checked with a party list (one proof), errpos and summary or not, with
// the scalar fields of bn254 and bls12-377:
//   * every region the form has starts at a multiple of 32, the regions lie in order and do not overlap,
//   * the total is what each of the four forms asked for before there was one layout function (written out below),
//   * one proof has no staging regions.
// Prints one line per violation, then "layouts N", "batches B rows R" and "V violations".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "curves.hpp"
#include "gao.hpp"
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

static size_t up32(size_t v) { return (v + 31) / 32 * 32; }

template <class F>
static size_t check_layouts() {
  size_t count = 0;
  const size_t elem = sizeof(F), sizes[4] = {1, 4, 512, (size_t)1 << 17};
  for (size_t nb = 1; nb <= (size_t)H_BATCH_MAX; nb++)
    for (int n = 4; n <= 32; n *= 2)
      for (size_t Lc : sizes)
        for (int form = 0; form < 9; form++) {
          // form 0: unchecked; 1..4: checked, bit 0 of form - 1 errpos, bit 1 summary; 5..8: the same with a party list
          const bool checked = form > 0, listed = form > 4, errpos = checked && ((form - 1) & 1), summary = checked && ((form - 1) & 2);
          if (listed && nb > 1) continue;
          count++;
          const size_t per = (size_t)n * Lc, vec = 6 * per * nb * elem;
          const size_t gao = checked ? gao_layout<F>(n, 3 * (int)nb, Lc, listed).bytes : 0;
          // what the four forms passed to hwork.ensure
          size_t want;
          if (!checked) {
            want = 6 * per * nb * sizeof(F);
          } else if (nb == 1 && !listed) {
            want = 6 * per * sizeof(F) + gao_layout<F>(n, 3, Lc, false).bytes;
          } else if (nb == 1) {
            want = 6 * per * sizeof(F) + gao_layout<F>(n, 3, Lc, true).bytes;
          } else {
            const size_t rows = (size_t)H_REPORT_ROWS * nb, sumw = (size_t)(3 + n);
            const size_t off_st = 6 * per * nb * sizeof(F) + up32(gao_layout<F>(n, 3 * (int)nb, Lc, false).bytes);
            const size_t off_ep = off_st + up32(rows * Lc);
            const size_t off_sm = off_ep + up32(errpos ? rows * Lc * 4 : 0);
            want = off_sm + (summary ? rows * sumw * 8 : 0);
          }
          const HLayout w = h_layout((size_t)n, nb, Lc, elem, gao, errpos, summary);
          CHECK(w.bytes == want, "nb %zu n %d Lc %zu form %d: %zu bytes, not %zu", nb, n, Lc, form, w.bytes, want);
          const size_t rows = checked && nb > 1 ? (size_t)H_REPORT_ROWS * nb : 0;
          const size_t start[6] = {0, w.w1, w.gao, w.status, w.errpos, w.summary};
          const size_t size[6] = {vec / 2, vec / 2, gao, rows * Lc, errpos ? rows * Lc * 4 : 0, summary ? rows * (3 + n) * 8 : 0};
          size_t end = 0;
          for (int r = 0; r < 6; r++) {
            if (!size[r]) continue;
            CHECK(start[r] % 32 == 0, "nb %zu n %d Lc %zu form %d: region %d starts at %zu", nb, n, Lc, form, r, start[r]);
            CHECK(start[r] >= end, "nb %zu n %d Lc %zu form %d: region %d at %zu overlaps the one before, which ends at %zu", nb, n,
                  Lc, form, r, start[r], end);
            end = start[r] + size[r];
          }
          // (the total keeps the padding behind a last region that is status or errpos rows)
          CHECK(end <= w.bytes && w.bytes - end < 32, "nb %zu n %d Lc %zu form %d: the regions end at %zu of %zu", nb, n, Lc, form, end,
                w.bytes);
          if (nb == 1)
            CHECK(w.status == w.bytes && w.errpos == w.bytes && w.summary == w.bytes, "n %d Lc %zu form %d: staging for one proof",
                  n, Lc, form);
        }
  return count;
}

int main() {
  std::printf("layouts %zu\n", check_layouts<Fp<Bn254Fr>>() + check_layouts<Fp<Bls377Fr>>());
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
