// Stand-alone test of csrc/party_rdv.hpp (the rendezvous behind zk_party_*): built plain, with -fsanitize=thread and with
// -fsanitize=address,undefined by tests/test_native_party.py.  No GPU, no HIP.
//   party_rdv_test rounds K     K parties x 3 slots, one thread per (party, slot), 200 rounds each, random arrival order
//   party_rdv_test mismatch     one differing record: BAD_INPUT for everyone, the right party named, the next round works
//   party_rdv_test timeout      50 ms timeout, one party stays away: PROTOCOL with its id, then the slot stays failed
//   party_rdv_test twice        a second thread inside the same (party, slot): BAD_INPUT; a stale sequence number likewise
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "party_rdv.hpp"

using namespace zk;
using clk = std::chrono::steady_clock;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static PartyRec rec_for(int party, int slot, uint64_t round) {
  PartyRec r;
  r.op = 1 + slot;
  r.log2_m = 10 + (int)(round % 7);
  r.len = 1000 + round;
  r.seed = 77 * round + slot;
  r.rearrange = (int)(round & 1);
  r.g_len = 32;
  for (int i = 0; i < 32; i++) r.g[i] = (unsigned char)(round + i);
  r.null_bits = round % 3;
  r.ptr[0] = (const void*)(uintptr_t)(0x1000 + party);      // not compared: differs per party by design
  r.caller = (void*)(uintptr_t)(party + 1);
  return r;
}

static int test_rounds(int k) {
  const int NSLOT = 3, ROUNDS = 200;
  std::vector<int> ids(k);
  for (int i = 0; i < k; i++) ids[i] = 8 + 2 * i;           // global ids are not the local indices
  PartySlot slot[NSLOT];
  for (auto& s : slot) s.init(k, ids.data());
  std::atomic<int> issued[NSLOT][ROUNDS];
  for (auto& a : issued)
    for (auto& b : a) b.store(0);
  std::atomic<int> bad{0};
  std::vector<std::thread> th;
  for (int s = 0; s < NSLOT; s++)
    for (int p = 0; p < k; p++)
      th.emplace_back([&, s, p] {
        std::mt19937 rng(1000 * s + p);
        for (uint64_t r = 0; r < (uint64_t)ROUNDS; r++) {
          if (rng() & 3) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 200));     // random arrival order
          PartyResult res = slot[s].arrive(p, r, rec_for(p, s, r), 20000, 20000, [&](const PartyRec* recs) {
            issued[s][r].fetch_add(1);
            for (int i = 0; i < k; i++) {                   // k records, in party order, of THIS round
              if (recs[i].ptr[0] != (const void*)(uintptr_t)(0x1000 + i) || recs[i].caller != (void*)(uintptr_t)(i + 1)) bad++;
              if (recs[i].len != 1000 + r || recs[i].op != 1 + s) bad++;
            }
            PartyResult out;
            out.code = (r % 5 == 4) ? ZK_ERR_GENERIC : ZK_OK;  // every caller must see the callback's code
            out.party = (int)r;
            out.msg = "round " + std::to_string(r);
            return out;
          });
          if (res.code != ((r % 5 == 4) ? ZK_ERR_GENERIC : ZK_OK) || res.party != (int)r || res.msg != "round " + std::to_string(r) ||
              !res.counted)
            bad++;
        }
      });
  for (auto& t : th) t.join();
  CHECK(bad.load() == 0);
  for (int s = 0; s < NSLOT; s++) {
    CHECK(slot[s].rounds() == (uint64_t)ROUNDS && !slot[s].failed());
    for (int r = 0; r < ROUNDS; r++) CHECK(issued[s][r].load() == 1);       // exactly once per round
  }
  printf("rounds k=%d: %d slots x %d rounds, one issue per round, records in party order\n", k, NSLOT, ROUNDS);
  return 0;
}

static int test_mismatch() {
  const int k = 8;
  int ids[k];
  for (int i = 0; i < k; i++) ids[i] = 16 + i;
  PartySlot slot;
  slot.init(k, ids);
  std::atomic<int> issued{0};
  for (int what = 0; what < 6; what++) {
    // round 2 * what: party 3 (and, in one round, party 5 as well: the LOWEST is named) differs in one field; round 2 * what + 1 is clean
    for (int clean = 0; clean < 2; clean++) {
      const uint64_t round = 2 * what + clean;
      std::vector<PartyResult> res(k);
      std::vector<std::thread> th;
      for (int p = 0; p < k; p++)
        th.emplace_back([&, p] {
          PartyRec r = rec_for(p, 0, round);
          if (!clean && (p == 3 || (what == 5 && p == 5))) {
            if (what == 0) r.log2_m++;
            if (what == 1) r.len++;
            if (what == 2) r.seed ^= 1;
            if (what == 3) r.g[31] ^= 0x80;
            if (what == 4) r.null_bits ^= 2;
            if (what == 5) r.rearrange ^= 1, r.group = 1;
          }
          res[p] = slot.arrive(p, round, r, 20000, 20000, [&](const PartyRec*) {
            issued++;
            return PartyResult();
          });
        });
      for (auto& t : th) t.join();
      for (int p = 0; p < k; p++) {
        CHECK(res[p].counted);
        if (clean) CHECK(res[p].code == ZK_OK);
        else CHECK(res[p].code == ZK_ERR_BAD_INPUT && res[p].party == 16 + 3 && res[p].msg.find("party 19") != std::string::npos);
      }
    }
  }
  CHECK(issued.load() == 6);          // the callback ran for the clean rounds only
  CHECK(!slot.failed());
  printf("mismatch: BAD_INPUT for all 8 callers, party 19 named, the callback did not run, the next round worked\n");
  return 0;
}

static int test_timeout() {
  const int k = 4;
  const int ids[k] = {4, 5, 6, 7};
  PartySlot slot;
  slot.init(k, ids);
  // a clean round first, so that the failed round is not the slot's first
  {
    std::vector<std::thread> th;
    std::atomic<int> ok{0};
    for (int p = 0; p < k; p++)
      th.emplace_back([&, p] { ok += slot.arrive(p, 0, rec_for(p, 0, 0), 50, 20000, [](const PartyRec*) { return PartyResult(); }).code == ZK_OK; });
    for (auto& t : th) t.join();
    CHECK(ok.load() == k);
  }
  std::vector<PartyResult> res(k);
  std::vector<double> ms(k, 0.0);
  std::atomic<int> issued{0};
  std::vector<std::thread> th;
  for (int p = 0; p < k; p++) {
    if (p == 2) continue;             // party 6 stays away
    th.emplace_back([&, p] {
      const auto t0 = clk::now();
      res[p] = slot.arrive(p, 1, rec_for(p, 0, 1), 50, 20000, [&](const PartyRec*) {
        issued++;
        return PartyResult();
      });
      ms[p] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    });
  }
  for (auto& t : th) t.join();
  for (int p = 0; p < k; p++) {
    if (p == 2) continue;
    CHECK(res[p].code == ZK_ERR_PROTOCOL && res[p].party == 6);
    CHECK(ms[p] < 5000.0);            // within the deadline (the bound allows for a loaded sanitizer build)
  }
  CHECK(ms[0] >= 45.0 || ms[1] >= 45.0 || ms[3] >= 45.0);     // and not before it: whoever arrived first waited it out
  CHECK(issued.load() == 0 && slot.failed());
  // the late arrival, and a caller of a later round: PROTOCOL at once, and the slot stays failed
  for (int again = 0; again < 2; again++) {
    const auto t0 = clk::now();
    // (a timeout of 20 s here: a return within a quarter of it shows that no wait was entered, however loaded the box is)
    PartyResult late = slot.arrive(2, 1 + again, rec_for(2, 0, 1 + again), 20000, 20000, [&](const PartyRec*) {
      issued++;
      return PartyResult();
    });
    const double t = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    CHECK(late.code == ZK_ERR_PROTOCOL && late.party == 6 && !late.counted && t < 5000.0);
  }
  CHECK(issued.load() == 0 && slot.failed());
  printf("timeout: PROTOCOL naming party 6 after %.0f / %.0f / %.0f ms; late arrivals refused at once\n", ms[0], ms[1], ms[3]);
  return 0;
}

static int test_twice() {
  const int k = 2;
  const int ids[k] = {0, 1};
  PartySlot slot;
  slot.init(k, ids);
  PartyResult first, second, stale, other;
  std::atomic<int> admitted{0};      // the admit hook runs for callers the round takes in, and for nobody else
  auto admit = [&] {
    admitted++;
    return true;
  };
  auto issue = [](const PartyRec*) { return PartyResult(); };
  std::thread a([&] { first = slot.arrive(0, 0, rec_for(0, 0, 0), 20000, 20000, issue, admit); });
  // once the first thread is inside, a second entry for the same party is refused (bounded poll: 20 s)
  for (int i = 0; slot.waiting() != 1; i++) {
    CHECK(i < 200000);
    std::this_thread::sleep_for(std::chrono::microseconds(100));
  }
  second = slot.arrive(0, 0, rec_for(0, 0, 0), 20000, 20000, issue, admit);
  CHECK(second.code == ZK_ERR_BAD_INPUT && !second.counted && second.party == 0 && admitted.load() == 1);
  stale = slot.arrive(1, 5, rec_for(1, 0, 0), 20000, 20000, issue, admit);
  CHECK(stale.code == ZK_ERR_BAD_INPUT && !stale.counted && stale.party == 1 && admitted.load() == 1);
  // a caller whose admit hook fails leaves again and may come back
  PartyResult unmarked = slot.arrive(1, 0, rec_for(1, 0, 0), 20000, 20000, issue, [] { return false; });
  CHECK(unmarked.code == ZK_ERR_GENERIC && !unmarked.counted && slot.waiting() == 1);
  other = slot.arrive(1, 0, rec_for(1, 0, 0), 20000, 20000, issue, admit);
  a.join();
  CHECK(admitted.load() == 2);
  CHECK(first.code == ZK_OK && first.counted && other.code == ZK_OK && other.counted);
  CHECK(slot.rounds() == 1 && !slot.failed());
  printf("twice: the second thread inside (party 0, slot) and a stale sequence number were refused; the round completed\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "rounds" && argc > 2) return test_rounds(atoi(argv[2]));
  if (mode == "mismatch") return test_mismatch();
  if (mode == "timeout") return test_timeout();
  if (mode == "twice") return test_twice();
  fprintf(stderr, "usage: party_rdv_test rounds K | mismatch | timeout | twice\n");
  return 2;
}
