// Host build of what every form of the robust unpack and the repair shares before a kernel runs (csrc/gao.hpp): the layout
// of the working memory (gao_layout), THE check of a party list (gao_list_check) and the refusals of a call (gao_call_check).
// Host only, checks itself: prints a line per failed expectation and returns their number (0: all good).
// tests/test_native_gao_batch_parties.py builds and runs it with the host compiler and once more under ASan + UBSan.
//   layout     nitems in {1, 3, 7} at n = 4 and n = 32, with and without tables, against the offsets the batch forms
//              always had, written out as constants (gao_batch_head / gao_batch_work_bytes / gao_batch_parties_work are
//              names over this one function now)
//   list       every refusal, in its order; lists of length 1, n - 1 and n at n = 4 and n = 32, given and null
//   call       every refusal of gao_call_check, in its order; no chunks is no refusal
#include <cstdio>
#include <cstring>
#include <vector>

#include "curves.hpp"
#include "gao.hpp"
using namespace zk;

static int bad = 0;
#define EXPECT(cond)                                          \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("line %d: %s\n", __LINE__, #cond);          \
      bad++;                                                  \
    }                                                         \
  } while (0)

static bool is(const GaoRefusal& r, int code, const char* msg) {
  return r.code == code && (msg ? r.msg && !std::strcmp(r.msg, msg) : r.msg == nullptr);
}
static const char* const COUNT = "bad party count";
static const char* const IDS = "party ids must be ascending and < n";
static const char* const DIM = "dimension must lie in 1 .. n - 1";
static const char* const FEW = "Not enough shares to reconstruct";

static void layout() {
  // n, nitems, nchunks, tab_size, inv_size -> tab (the end of the cleared head), inv, list, bytes
  static const size_t want[][9] = {
      {4, 1, 65, 0, 0, 96, 96, 96, 356},
      {4, 1, 65, 3724, 1024, 96, 3840, 4864, 5124},
      {4, 3, 65, 0, 0, 224, 224, 224, 1004},
      {4, 3, 65, 3724, 1024, 224, 3968, 4992, 5772},
      {4, 7, 65, 0, 0, 448, 448, 448, 2268},
      {4, 7, 65, 3724, 1024, 448, 4192, 5216, 7036},
      {32, 1, 65, 0, 0, 320, 320, 320, 580},
      {32, 1, 65, 3724, 1024, 320, 4064, 5088, 5348},
      {32, 3, 65, 0, 0, 896, 896, 896, 1676},
      {32, 3, 65, 3724, 1024, 896, 4640, 5664, 6444},
      {32, 7, 65, 0, 0, 2016, 2016, 2016, 3836},
      {32, 7, 65, 3724, 1024, 2016, 5760, 6784, 8604},
  };
  for (const auto& w : want) {
    const GaoLayout g = gao_layout((int)w[0], (int)w[1], w[2], w[3], w[4]);
    EXPECT(g.tab == w[5] && g.inv == w[6] && g.list == w[7] && g.bytes == w[8]);
    EXPECT(g.tab >= 32 + w[1] * (3 + w[0]) * 8);      // the count and every item's summary words lie in the head
  }
  // the typed form: the tables' real sizes, present only with a list, the inverses only for a repair
  using F = Fp<Bn254Fr>;
  const size_t tab = sizeof(GaoAbsent<F>), inv = sizeof(GaoInvLambda<F>);
  for (int nitems : {1, 3, 7}) {
    const GaoLayout none = gao_layout<F>(32, nitems, 65, false), both = gao_layout<F>(32, nitems, 65, true),
                    unpack = gao_layout<F>(32, nitems, 65, true, false);
    const GaoLayout raw0 = gao_layout(32, nitems, 65, 0, 0), raw2 = gao_layout(32, nitems, 65, tab, inv),
                    raw1 = gao_layout(32, nitems, 65, tab, 0);
    EXPECT(!std::memcmp(&none, &raw0, sizeof(none)) && !std::memcmp(&both, &raw2, sizeof(both)) &&
           !std::memcmp(&unpack, &raw1, sizeof(unpack)));
    EXPECT(both.inv - both.tab >= tab && both.list - both.inv >= inv && unpack.list == unpack.inv);
  }
}

static void lists() {
  for (int n : {4, 32}) {
    const int k = n / 2;
    std::vector<uint32_t> all((size_t)n);
    for (int i = 0; i < n; i++) all[(size_t)i] = (uint32_t)i;
    // ---- lists that pass: n, n - 1 (each party left out once), and 1 with ids_only or dimension... 1 is too few shares
    for (const uint32_t* given : {(const uint32_t*)all.data(), (const uint32_t*)nullptr}) {
      uint32_t ids[GAO_MAX_N];
      std::memset(ids, 0xff, sizeof(ids));
      EXPECT(is(gao_list_check(given, n, k, n, ids), ZK_OK, nullptr));
      for (int i = 0; i < n; i++) EXPECT(ids[i] == (uint32_t)i);
      EXPECT(is(gao_list_check(given, n - 1, k, n, ids), ZK_OK, nullptr));      // (null: 0 .. n - 2)
      EXPECT(is(gao_list_check(given, 1, k, n, ids), ZK_ERR_PROTOCOL, FEW));
      EXPECT(is(gao_list_check(given, 1, k, n, ids, true), ZK_OK, nullptr));
    }
    for (int out = 0; out < n; out++) {
      std::vector<uint32_t> s;
      for (int i = 0; i < n; i++)
        if (i != out) s.push_back((uint32_t)i);
      uint32_t ids[GAO_MAX_N];
      EXPECT(is(gao_list_check(s.data(), n - 1, n - 2, n, ids), ZK_OK, nullptr));
      EXPECT(!std::memcmp(ids, s.data(), s.size() * 4));
      EXPECT(is(gao_list_check(s.data(), n - 1, n - 1, n, ids), ZK_ERR_PROTOCOL, FEW));
    }
    for (uint32_t one : {0u, (uint32_t)n - 1}) {      // a list of one party: the ids pass, any dimension leaves too few shares
      uint32_t ids[GAO_MAX_N];
      EXPECT(is(gao_list_check(&one, 1, 1, n, ids), ZK_ERR_PROTOCOL, FEW) && ids[0] == one);
      EXPECT(is(gao_list_check(&one, 1, 1, n, ids, true), ZK_OK, nullptr));
    }
    // ---- every refusal, and which one wins when several apply: count, ids, dimension, too few shares
    uint32_t ids[GAO_MAX_N];
    std::vector<uint32_t> v = all;
    EXPECT(is(gao_list_check(v.data(), 0, 0, n, ids), ZK_ERR_BAD_INPUT, COUNT));
    EXPECT(is(gao_list_check(v.data(), -1, k, n, ids), ZK_ERR_BAD_INPUT, COUNT));
    EXPECT(is(gao_list_check(nullptr, n + 1, k, n, ids), ZK_ERR_BAD_INPUT, COUNT));      // (ids holds GAO_MAX_N: never written)
    v[1] = (uint32_t)n;                                                                  // an id that is not below n
    EXPECT(is(gao_list_check(v.data(), 2, 0, n, ids), ZK_ERR_BAD_INPUT, IDS));
    v[1] = 0;                                                                            // a repeated id
    EXPECT(is(gao_list_check(v.data(), 2, 1, n, ids), ZK_ERR_BAD_INPUT, IDS));
    v[0] = 2, v[1] = 1;                                                                  // descending
    EXPECT(is(gao_list_check(v.data(), 3, n, n, ids, true), ZK_ERR_BAD_INPUT, IDS));
    v[0] = 0xffffffffu;                                                                  // (no wrap into a valid id)
    EXPECT(is(gao_list_check(v.data(), 1, 1, n, ids), ZK_ERR_BAD_INPUT, IDS));
    EXPECT(is(gao_list_check(all.data(), n, 0, n, ids), ZK_ERR_BAD_INPUT, DIM));
    EXPECT(is(gao_list_check(all.data(), n, n, n, ids), ZK_ERR_BAD_INPUT, DIM));
    EXPECT(is(gao_list_check(all.data(), 1, n, n, ids), ZK_ERR_BAD_INPUT, DIM));         // ahead of too few shares
    EXPECT(is(gao_list_check(all.data(), n, n - 1, n, ids), ZK_OK, nullptr));
    EXPECT(is(gao_list_check(all.data(), k, k, n, ids), ZK_ERR_PROTOCOL, FEW));
    EXPECT(is(gao_list_check(all.data(), k + 1, k, n, ids), ZK_OK, nullptr));
    EXPECT(is(gao_list_check(all.data(), n, 0, n, ids, true), ZK_OK, nullptr));          // ids_only: the dimension is not read
  }
}

static void calls() {
  static const char* const RANGE = "bad range: cnt <= stride < 2^32, cnt <= len, base < len, shift <= len";
  for (int l : {1, 8}) {
    const int n = 4 * l;
    uint32_t ids[GAO_MAX_N];
    char sh, stt;
    GaoCall c;
    c.shares = &sh, c.status = (uint8_t*)&stt, c.np = n, c.nchunks = 5, c.dimension = 2 * l;
    EXPECT(is(gao_call_check(l, c, false, ids), ZK_OK, nullptr) && is(gao_call_check(l, c, true, ids), ZK_OK, nullptr));
    EXPECT(c.pitch() == 5 && !c.batch());
    EXPECT(is(gao_call_check(3, c, true, ids), ZK_ERR_BAD_INPUT, "packing factor l must be 1, 2, 4 or 8"));
    GaoCall d = c;
    d.dimension = n;
    EXPECT(is(gao_call_check(l, d, true, ids), ZK_ERR_BAD_INPUT, DIM));
    d.np = n + 1;
    EXPECT(is(gao_call_check(l, d, true, ids), ZK_ERR_BAD_INPUT, COUNT));
    d = c, d.shares = nullptr;
    EXPECT(is(gao_call_check(l, d, true, ids), ZK_ERR_BAD_INPUT, "null pointer"));
    d.nchunks = 0;                                       // no chunks: the pointers are not looked at
    EXPECT(is(gao_call_check(l, d, true, ids), ZK_OK, nullptr));
    d.dimension = 0;                                     // but the list and the dimension are
    EXPECT(is(gao_call_check(l, d, true, ids), ZK_ERR_BAD_INPUT, DIM));
    d = c, d.status = nullptr;
    EXPECT(is(gao_call_check(l, d, false, ids), ZK_ERR_BAD_INPUT, "null pointer"));
    d = c, d.nchunks = (size_t)1 << 32;
    EXPECT(is(gao_call_check(l, d, true, ids), ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks"));
    d.nchunks = ((size_t)1 << 32) - 1;
    EXPECT(is(gao_call_check(l, d, true, ids), ZK_OK, nullptr));
    // ---- the range form: a repair of one word; the range is refused ahead of everything else
    GaoRange rg{8, 5, 3, 1, 9};                          // stride, cnt, base, shift, len
    d = c, d.range = &rg;
    EXPECT(is(gao_call_check(l, d, true, ids), ZK_OK, nullptr) && d.pitch() == 8);
    EXPECT(gao_call_check(l, d, false, ids).code == ZK_ERR_BAD_INPUT);
    d.np = 0;
    for (const GaoRange& b : {GaoRange{4, 5, 3, 1, 9}, GaoRange{8, 5, 3, 1, 4}, GaoRange{8, 5, 9, 1, 9}, GaoRange{8, 5, 3, 10, 9},
                              GaoRange{(size_t)1 << 32, 5, 3, 1, 9}, GaoRange{8, 0, 0, 0, 0}}) {
      d.range = &b, d.nchunks = b.len ? 5 : 1;           // (the last: a good empty range with a count that is not its cnt)
      EXPECT(is(gao_call_check(l, d, true, ids), ZK_ERR_BAD_INPUT, RANGE));
    }
    GaoRange empty{8, 0, 0, 0, 0};
    d = c, d.range = &empty, d.nchunks = 0, d.shares = nullptr;
    EXPECT(is(gao_call_check(l, d, true, ids), ZK_OK, nullptr));
    // ---- a batch
    d = c, d.nitems = 3, d.item_stride = (size_t)n * 5 + 2;
    EXPECT(d.batch() && is(gao_call_check(l, d, true, ids), ZK_OK, nullptr));
    d.range = &rg;
    EXPECT(gao_call_check(l, d, true, ids).code == ZK_ERR_BAD_INPUT);
  }
}

int main() {
  layout();
  lists();
  calls();
  std::printf("%d failed\n", bad);
  return bad > 255 ? 255 : bad;
}
