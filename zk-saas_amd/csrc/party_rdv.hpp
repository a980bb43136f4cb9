// The rendezvous behind the per-party entry points (zk_party_*): one slot per (net, sid) turns the k local callers of a
// round -- one host thread per party, as mpc-net/src/multi.rs:301-328 runs one task per party -- into the ONE rank call
// (zk_dist_*) that exists.  Host only: plain C++17, no HIP and no engine types, so that it compiles into a stand-alone test
// program (tests/native/party_rdv_test.cpp) the way hostpool.hpp and net.hpp's host mode do.
//
//   arrive(local party index, sequence number, record) collects k records of one sequence number and hands them, in
//   ascending party order, to the issue callback: exactly once, on the thread that arrived last, with no lock of this
//   header held.  Every one of the k callers returns the callback's code, message and party.
//
//   Agreement   the fields of a record the rank call takes ONCE must be equal across the k records; otherwise every caller
//               of the round gets ZK_ERR_BAD_INPUT naming the lowest party that differs from the rank's first party, and the
//               callback does not run (nothing has entered the net round: the net stays usable, the next round works).
//   Deadline    a waiter waits at most `timeout_ms` for the other parties; on expiry every waiter of that round returns
//               ZK_ERR_PROTOCOL with the lowest missing party's id and the slot is FAILED: a caller that arrives later, for
//               that round or a later one, gets ZK_ERR_PROTOCOL at once.  While the callback runs nobody is missing: the
//               waiters then wait at most `issue_ms` (the bound of what the rank call itself may wait for), and an expiry
//               fails the slot in the same way.  No wait in this header is unbounded.
//   One channel, one party   a second thread inside the same (party, slot) gets ZK_ERR_BAD_INPUT.
//   Sequence    a caller's per-(party, slot) number must be the number of rounds this slot has finished; otherwise
//               ZK_ERR_BAD_INPUT for that caller alone.  The number belongs to the PARTY, not to a handle: whoever owns the
//               slots keeps one counter per (party, slot), so that any handle of a party continues where the last one stopped.
// Two rounds can be alive at once (the waiters of round N still leaving while the first caller of N + 1 arrives; N + 2 cannot
// begin before everyone has left N, because it needs everyone's arrival in N + 1), hence the two round records.
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/zksaas.h"

namespace zk {

constexpr int PARTY_MAXK = 32;       // parties of one rank
constexpr int PARTY_NPTR = 40;       // the prover's operands: 5 CRS vectors, 5 share vectors, 14 + 10 mask rows, 3 outputs

struct PartyRec {
  // ---- compared: what the rank call takes once
  int op = 0, log2_m = 0, rearrange = 0, group = 0;
  uint64_t len = 0, seed = 0, ext[3] = {0, 0, 0};
  uint64_t null_bits = 0;            // bit i: pointer i of the call is NULL (masks: NULL = the zero mask)
  uint32_t g_len = 0;
  unsigned char g[96] = {0};         // the bytes of g (d_ifft) or of r | s (the prover)
  // ---- not compared: this party's rows and whatever the issuer needs of the caller (its stream, its event, its handle)
  const void* ptr[PARTY_NPTR] = {nullptr};
  void* caller = nullptr;            // caller-owned memory the issuer reads BEFORE the rank call only (the prover's CRS struct)
  void* h[2] = {nullptr, nullptr};   // opaque handles, copied: the caller's stream and the event it recorded on arrival

  bool agrees(const PartyRec& o) const {
    return op == o.op && log2_m == o.log2_m && rearrange == o.rearrange && group == o.group && len == o.len && seed == o.seed &&
           ext[0] == o.ext[0] && ext[1] == o.ext[1] && ext[2] == o.ext[2] && null_bits == o.null_bits && g_len == o.g_len &&
           memcmp(g, o.g, sizeof g) == 0;
  }
};

struct PartyResult {
  int code = ZK_OK;
  int party = -1;
  std::string msg;
  bool counted = false;      // the result of a ROUND (it used up a sequence number), not a refusal of this caller alone
};

class PartySlot {
 public:
  // ids: the global ids of this rank's k parties, ascending (messages name them)
  void init(int k, const int* ids) {
    std::lock_guard<std::mutex> lk(mu_);
    k_ = k;
    for (int i = 0; i < k && i < PARTY_MAXK; i++) ids_[i] = ids[i];
  }
  uint64_t rounds() const {
    std::lock_guard<std::mutex> lk(mu_);
    return base_;
  }
  bool failed() const {
    std::lock_guard<std::mutex> lk(mu_);
    return failed_;
  }
  int waiting() const {        // callers inside the round that is collecting
    std::lock_guard<std::mutex> lk(mu_);
    return rounds_[base_ & 1].arrived;
  }

  // Issue: PartyResult(const PartyRec* recs /* k, ascending party order */)
  template <class Issue>
  PartyResult arrive(int p, uint64_t seq, const PartyRec& rec, uint64_t timeout_ms, uint64_t issue_ms, Issue&& issue) {
    return arrive(p, seq, rec, timeout_ms, issue_ms, issue, [] { return true; });
  }
  // Admit: bool(), run once the caller is ADMITTED to the round (not for a refused second thread or a stale number), before
  // anybody can issue, with this slot's lock held: it must be short and must not call back into the slot.  false = the caller
  // could not mark its arrival: it leaves the round again with ZK_ERR_GENERIC.
  template <class Issue, class Admit>
  PartyResult arrive(int p, uint64_t seq, const PartyRec& rec, uint64_t timeout_ms, uint64_t issue_ms, Issue&& issue,
                     Admit&& admit) {
    using clock = std::chrono::steady_clock;
    std::unique_lock<std::mutex> lk(mu_);
    if (failed_) {
      PartyResult r = fail_;
      r.counted = false;
      return r;
    }
    if (k_ < 1 || k_ > PARTY_MAXK || p < 0 || p >= k_) return result(ZK_ERR_BAD_INPUT, "party: not a party of this rank", -1);
    Round& R = rounds_[base_ & 1];
    if (R.have[p])
      return result(ZK_ERR_BAD_INPUT, "party " + std::to_string(ids_[p]) + ": two threads inside the same (party, sid)", ids_[p]);
    if (seq != base_)
      return result(ZK_ERR_BAD_INPUT, "party " + std::to_string(ids_[p]) + ": call " + std::to_string(seq) +
                                          " of this handle on a channel that has finished " + std::to_string(base_) + " rounds",
                    ids_[p]);
    if (!admit()) return result(ZK_ERR_GENERIC, "party " + std::to_string(ids_[p]) + ": could not mark its arrival", ids_[p]);
    R.have[p] = true;
    R.rec[p] = rec;
    R.arrived++;
    if (R.arrived == k_) {
      int bad = -1;
      for (int i = 1; i < k_ && bad < 0; i++)
        if (!R.rec[i].agrees(R.rec[0])) bad = i;
      if (bad >= 0) {
        R.res = result(ZK_ERR_BAD_INPUT, "party " + std::to_string(ids_[bad]) + " passed other arguments than party " +
                                             std::to_string(ids_[0]) + " in the same round (log2_m, len, rearrange, seed, group, g, NULL masks)",
                       ids_[bad]);
      } else {
        R.issuing = true;
        lk.unlock();
        PartyResult r = issue((const PartyRec*)R.rec);      // nobody writes R.rec while have[] is full
        lk.lock();
        R.issuing = false;
        if (failed_) r = fail_;                              // a waiter gave up on the issuer: everyone reports that
        R.res = r;
      }
      R.res.counted = true;
      R.done = true;
      base_++;
      cv_.notify_all();
      return leave(R);
    }
    auto dl = clock::now() + std::chrono::milliseconds(timeout_ms);
    bool issue_seen = false;
    for (;;) {
      if (R.done) return leave(R);
      if (failed_) {
        PartyResult r = fail_;
        leave(R);
        return r;
      }
      if (R.issuing && !issue_seen) {
        // everyone is here and the rank call runs: bounded by what the rank call itself may wait for, counted from now
        issue_seen = true;
        dl = clock::now() + std::chrono::milliseconds(issue_ms);
      }
      if (cv_.wait_until(lk, dl) != std::cv_status::timeout) continue;
      if (R.done || failed_ || (R.issuing && !issue_seen) || clock::now() < dl) continue;
      int missing = -1;
      for (int i = 0; i < k_ && missing < 0; i++)
        if (!R.have[i]) missing = i;
      failed_ = true;
      if (missing >= 0)
        fail_ = result(ZK_ERR_PROTOCOL, "party " + std::to_string(ids_[missing]) + " did not join the round within " +
                                            std::to_string(timeout_ms) + " ms: the rank did not enter it (rebuild the net)",
                       ids_[missing]);
      else
        fail_ = result(ZK_ERR_PROTOCOL, "the rank call did not return within " + std::to_string(issue_ms) + " ms (rebuild the net)",
                       ids_[0]);
      fail_.counted = true;
      R.res = fail_;
      if (!R.issuing) R.done = true, base_++;      // (an issuer that is still out finishes the round itself)
      cv_.notify_all();
    }
  }

 private:
  struct Round {
    bool have[PARTY_MAXK] = {false};
    PartyRec rec[PARTY_MAXK];
    int arrived = 0, left = 0;
    bool done = false, issuing = false;
    PartyResult res;
  };
  static PartyResult result(int code, const std::string& m, int party) {
    PartyResult r;
    r.code = code;
    r.msg = m;
    r.party = party;
    return r;
  }
  // called with the lock held by everyone who arrived in R; the last one out clears the record for round N + 2
  PartyResult leave(Round& R) {
    PartyResult r = R.res;
    if (++R.left == R.arrived && R.done) {
      for (int i = 0; i < PARTY_MAXK; i++) R.have[i] = false;
      R.arrived = R.left = 0;
      R.done = false;
      R.res = PartyResult();
    }
    return r;
  }
  mutable std::mutex mu_;
  std::condition_variable cv_;
  int k_ = 0;
  int ids_[PARTY_MAXK] = {0};
  uint64_t base_ = 0;          // rounds finished = the sequence number the next round carries
  bool failed_ = false;
  PartyResult fail_;
  Round rounds_[2];
};

}  // namespace zk
