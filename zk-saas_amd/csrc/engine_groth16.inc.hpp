// Part of class Engine<Cfg> (engine_impl.hpp includes this file INSIDE the class body): the Groth16 prover (one proof, two in flight) and the batch prover (the h chain: engine_h.inc.hpp).
// Split out of engine_impl.hpp in round 5 (one 3 400-line class body had stopped being navigable); not a stand-alone header.

  // ---------------------------------------------------------------- prover (prove.rs, sha256.rs:32-129)
  // Everything the host contributes to a proof (scalar multiples of CRS constants, of the out-masks and of the in-mask
  // sums, MSM window folds) is a task of the context's persistent pool, submitted when the proof starts and running
  // beside the device work (the overlap the reference gets from tokio::try_join!, prove.rs:209-227); the end of a proof
  // only adds points.  The bookkeeping is split by what it belongs to:
  //   ProofTerms   ONE proof, whatever launched it: its inputs, the MSM results and every host term;
  //   JobCore      ONE set of MSM chains in flight: workspace slots, pending launches, scratch, pool tasks, events;
  //   ProveJob     JobCore + one ProofTerms (a single or a sharded proof); BatchJob: JobCore + nb ProofTerms.
  // Slot lookup, busy, drain, dump, abort, bail and join work on the JobCore, whichever kind of job it is part of.

  struct ProofTerms {
    zk_crs_share crs{};
    zk_groth16_masks mk{};
    bool has_mk = false, r_zero = false, full = true;
    int first = 0, count = 0;
    Fr r, s;
    P1 S, H, W, U, sS, rH;                          // (a full proof whose H and W launches donate their buckets to U's --
                                                    // prove_begin_impl "one bucket set for C" -- leaves H, W and rH the
                                                    // identity and U holds T = r*H + W + U)
    P2 V0;
    P1 rN, sK, rsM, s_cA, r_cB1;
    P2 sK2;
    P1 in1[5], s_in0, r_in1;                        // in-mask sums (index 2 unused) and their multiples
    P2 in2;
    std::vector<P1> s_om0, r_om1;                   // per party: s * out_mask_A[p], r * out_mask_B1[p]
    std::vector<Fr> coef;                           // a proof from a party list: the king's coefficients of the five MSM
                                                    // rounds by party id, [n], zero at an absent party (coefs_for); empty:
                                                    // all n parties, the MSM's own tables
    Status err;                                     // first failure reported by a task (tasks must not touch `last`)
    std::mutex emu;
    const zk_groth16_masks* masks() const { return has_mk ? &mk : nullptr; }
    const Fr* coefs() const { return coef.empty() ? nullptr : coef.data(); }
    MsmSums sums() const {
      return {xyzz_add_ni(S, in1[0]), r_zero ? P1::identity() : xyzz_add_ni(H, in1[1]), xyzz_add_ni(W, in1[3]),
              xyzz_add_ni(U, in1[4]), xyzz_add_ni(V0, in2)};
    }
  };
  struct JobCore {
    const bool is_batch;
    bool active = false;
    int slot = 0, ws0 = 0;                          // handle; workspace slot of role 0 (ws_job / ws_batch): set by Engine()
    MsmPending msm[NROLES];                         // by MsmRole (msm.hpp); workspace slots ws0 + role
    DevBuf hwork, hshare;
    std::vector<std::future<void>> fut;
    int rc[ROLE_U] = {};                            // results of the S+H, W and V tasks (U is folded by the join)
    hipEvent_t ev_in = nullptr;                     // orders the job's streams behind the caller's
    hipEvent_t ev_role[NROLES] = {};                // by MsmRole: behind the sort (a proof's "all sorts first" barrier,
                                                    // prove_begin_impl) or behind the accumulate kernel (a batch's chain)
    hipEvent_t ev_don = nullptr;                    // behind the finalize kernel of the S+H launch when H's buckets are donated
    std::atomic<int> don_flag[2] = {};              // the S+H / W launch has donated (1) or failed (-1): MsmShare::from_flag
    explicit JobCore(bool batch) : is_batch(batch) {}
    ~JobCore() {
      if (ev_in) (void)hipEventDestroy(ev_in);
      if (ev_don) (void)hipEventDestroy(ev_don);
      for (hipEvent_t e : ev_role)
        if (e) (void)hipEventDestroy(e);
    }
  };
  // One proof in flight.  `sharded`: started by zk_dist_groth16_prove_async for this rank's k parties -- the handle is
  // then joined by zk_dist_groth16_wait only (and released by zk_groth16_abort like any other).
  struct ProveJob : JobCore {
    ProveJob() : JobCore(false) {}
    ProofTerms pt;
    bool gate_sorts = false, sharded = false;
    DevBuf coef_d;                      // the device copy of pt.coef while the proof of a party list is in flight
    std::atomic<int> sorted_cnt{0};     // witness MSMs of this proof whose sort has been enqueued and recorded (MsmGate)
    int k = 0;
    uint32_t cmask3 = 0;
    // a checked proof (zk_groth16_prove_checked*_async): where its report goes and the validated party list -- the job's own
    // copies, so that nothing it reads after the call has returned belongs to the caller (report.ids points at report_ids)
    bool checked = false;
    HReport report{};
    uint32_t report_ids[GAO_MAX_N] = {};
  };
  ProveJob jobs_[NJOBS];
  // A batch of proofs against one CRS in flight (zk_groth16_prove_batch_async).  Each batch slot has its own MSM
  // workspaces, scratch and stream set, so that the sort phase of one batch runs under the accumulate kernels of the
  // other and the reduction tails of one under the other's accumulates -- one batch alone leaves the chip partly idle
  // for ~1 ms at either end.
  struct BatchJob : JobCore {
    BatchJob() : JobCore(true) {}
    int nb = 0;
    std::deque<ProofTerms> pt;                      // per proof (grows to the largest batch seen)
    bool own_streams = false;
    MsmGate gate_u;
    std::atomic<int> acc_flag[NROLES] = {};         // by role: the record of ev_role has been enqueued (MsmGate)
    hipStream_t st[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~BatchJob() {
      if (own_streams)
        for (hipStream_t s_ : st)
          if (s_) (void)hipStreamDestroy(s_);
    }
  };
  BatchJob bjobs_[NBATCH];

  static const char* kind(const JobCore& c) { return c.is_batch ? "batch" : "proof"; }
  static int nproofs(const JobCore& c) { return c.is_batch ? static_cast<const BatchJob&>(c).nb : 1; }
  static ProofTerms& terms(JobCore& c, int b) {
    return c.is_batch ? static_cast<BatchJob&>(c).pt[b] : static_cast<ProveJob&>(c).pt;
  }
  // the first free job of a kind, nullptr when all are in flight
  template <class Job, size_t N>
  static Job* free_job(Job (&jobs)[N]) {
    for (Job& j : jobs)
      if (!j.active) return &j;
    return nullptr;
  }
  // every handle is checked on its own: a failure half-way leaves the rest to be created by the next call
  int ensure_events(JobCore& c) {
    if (!c.ev_in) ZK_HIP(hipEventCreateWithFlags(&c.ev_in, hipEventDisableTiming));
    if (!c.ev_don) ZK_HIP(hipEventCreateWithFlags(&c.ev_don, hipEventDisableTiming));
    for (hipEvent_t& e : c.ev_role)
      if (!e) ZK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return ZK_OK;
  }

  static P1 aff1(const void* p) {
    Affine<Fq_> a;
    memcpy(&a, p, sizeof(a));
    return P1::from_affine(a);
  }
  static P2 aff2(const void* p) {
    Affine<Fq2_> a;
    memcpy(&a, p, sizeof(a));
    return P2::from_affine(a);
  }
  // ---- bounded waits (round 6, VERDICT r5 #10 / ADVICE r5): every wait of a job is bounded by the context's deadline
  // (engine.hpp wait_deadline_ms).  A wait that expires leaves device work or a pool task that still references the
  // job's buffers: the job's slot is then never reused (it stays `active`), the context is wedged (engine.hpp wedge)
  // and the state of every gate / event of the job goes to stderr.
  static const char* ev_state(hipEvent_t e) {
    if (!e) return "none";
    hipError_t q = hipEventQuery(e);
    return q == hipSuccess ? "done" : (q == hipErrorNotReady ? "PENDING" : hipGetErrorString(q));
  }
  MsmSlot& job_slot(const JobCore& c, int role) { return msm_.slots_[c.ws0 + role]; }
  // Slots whose launches donated buckets to the job's U launch stay busy beyond their own event (MsmSlot::lent): they are
  // released here, once the U chain has been waited for (or was never enqueued) and the job's pool tasks are joined.
  void release_loans(JobCore& c) {
    if (job_slot(c, ROLE_U).busy) return;
    for (int r : {(int)ROLE_SH, (int)ROLE_W})
      if (job_slot(c, r).lent) (void)job_slot(c, r).release_loan(this);
  }
  // once the job's tasks are joined, a busy slot is a wait that expired: its work may still run
  bool busy(const JobCore& c) {
    for (int r = 0; r < NROLES; r++)
      if (job_slot(c, r).busy) return true;
    return false;
  }
  // joins the pool tasks of a job; false = some did not finish within the deadline (they stay in `fut`)
  bool drain(JobCore& c) {
    const auto dl = deadline_from_now();
    for (auto& f : c.fut)
      if (f.valid() && f.wait_until(dl) != std::future_status::ready) return false;
    c.fut.clear();
    return true;
  }
  void dump(const char* who, const char* why, JobCore& c) {
    int np = 0;
    for (auto& f : c.fut)
      if (f.valid() && f.wait_for(std::chrono::seconds(0)) != std::future_status::ready) np++;
    fprintf(stderr, "[zksaas] %s: %s: %s slot %d (%d proofs): pool tasks pending %d", who, why, kind(c), c.slot, nproofs(c), np);
    if (!c.is_batch) fprintf(stderr, ", sorted_cnt %d", static_cast<ProveJob&>(c).sorted_cnt.load());
    fprintf(stderr, ";");
    for (int r = 0; r < NROLES; r++) {
      fprintf(stderr, " %s:", ROLE_NAME[r]);
      if (c.is_batch)
        fprintf(stderr, " launched-flag %d, accumulate event %s,", static_cast<BatchJob&>(c).acc_flag[r].load(), ev_state(c.ev_role[r]));
      fprintf(stderr, " chain event %s%s;", ev_state(job_slot(c, r).ev), job_slot(c, r).busy ? "" : " (idle)");
    }
    fprintf(stderr, "\n");
  }
  // joins a job's tasks and device work and marks it free (after an error, or zk_groth16_abort)
  void abort(JobCore& c) {
    // a proof's tasks waiting at the sort barrier go on (and fail or finish); a batch's gates are always raised (msm_task)
    if (!c.is_batch) static_cast<ProveJob&>(c).sorted_cnt.fetch_add(1 << 20, std::memory_order_release);
    bool ok = drain(c);
    ok = ok && job_slot(c, ROLE_U).wait(this) != hipErrorNotReady;
    if (ok) release_loans(c);
    for (int r = 0; r < NROLES; r++) ok = ok && job_slot(c, r).wait(this) != hipErrorNotReady;
    if (!ok) {
      dump("abort", "work of the job is still pending after the deadline", c);
      Status keep = last;
      wedge(std::string("a ") + kind(c) + " could not be aborted within the deadline (wait_deadline_ms): its slot is not reused");
      if (keep.code) last = keep;
      return;                                                        // stays active: nothing of it is reused
    }
    c.active = false;
  }
  // A failure after the job was marked active leaves pool tasks and MSMs in flight that reference the caller's buffers:
  // every such return aborts the job -- once -- and keeps the first error's message.
  int bail(JobCore& c, int rc) {
    Status keep = last;
    abort(c);
    last = keep;
    return rc;
  }
  int drain_or_wedge(JobCore& c, const char* who) {
    if (drain(c)) return ZK_OK;
    dump(who, "pool tasks did not finish within the deadline", c);
    return wedge(std::string(who) + ": host tasks of the " + kind(c) +
                 " did not finish within the deadline (wait_deadline_ms); the slot is not reused");
  }
  // The end of every job: folds U (always waited for, whatever failed before: its launch references the job's buffers)
  // into the proofs' terms, joins the pool tasks and frees the job -- unless a wait expired, which wedges the context.
  // `who`: the ABI call that joins.  Afterwards terms(c, b).sums() are the proofs' totals.
  int join(JobCore& c, const char* who) {
    P1 ures[MSM_MAXB];
    int rc = msm_fold_batch<Fq_>(this, c.msm[ROLE_U], ures, 1);
    Status keep = last;
    const bool expired = rc && job_slot(c, ROLE_U).busy;
    if (expired) dump(who, "the U-MSM chain did not finish within the deadline", c);
    if (int rd = drain_or_wedge(c, who)) return rd;
    release_loans(c);
    if (busy(c)) {                        // a chain's event did not signal within the deadline: nothing may be reused
      if (!expired) dump(who, "an MSM chain did not finish within the deadline", c);
      return wedge(expired ? keep.msg : std::string(last.msg));
    }
    c.active = false;
    if (rc) return rc;
    for (int e : c.rc)
      if (e) return e;      // a pool task failed: its message was recorded on the engine by msm_launch (hip_fail); keep it
    for (int b = 0; b < nproofs(c); b++) {
      ProofTerms& t = terms(c, b);
      if (t.err.code) return fail(t.err.code, t.err.msg);
      t.U = ures[b];
    }
    return ZK_OK;
  }
  // engine-level failure recorded from a pool task (IEngine::fail is not thread-safe)
  int task_fail(ProofTerms& t, int code, const std::string& msg) {
    std::lock_guard<std::mutex> lk(t.emu);
    if (t.err.code == ZK_OK) {
      t.err.code = code;
      t.err.msg = msg;
    }
    return code;
  }

  void init_terms(ProofTerms& j, const zk_crs_share* crs, const zk_groth16_masks* mk, const Fr& r, const Fr& s, bool full,
                  int first, int count) {
    j.crs = *crs;
    j.has_mk = mk != nullptr;
    j.mk = mk ? *mk : zk_groth16_masks{};
    j.r = r;
    j.s = s;
    j.r_zero = r.is_zero();
    j.full = full;
    j.first = first;
    j.count = count;
    j.err = Status{};
    j.coef.clear();
    j.S = j.H = j.W = j.U = j.sS = j.rH = j.s_in0 = j.r_in1 = P1::identity();
    j.V0 = j.in2 = P2::identity();
    for (int k = 0; k < 5; k++) j.in1[k] = P1::identity();
    j.s_om0.assign(n, P1::identity());
    j.r_om1.assign(n, P1::identity());
  }
  // One witness MSM of a job as a pool task: it enqueues the launch (a dozen kernel launches) on workspace slot
  // ws0 + role, waits for the slot's event, folds the windows on the host and hands the points to then(res), res =
  // [base vector][scalar vector].  Whatever waits on this launch is released also when it failed early (waiters must not
  // hang): a batch raises `raise` (its accumulate-order flag of the role) in any case, a proof counts a failed launch into
  // its sort barrier.  batch: the scalar vectors of a batched launch (copied), else `scal`.
  template <class Fld, class Then>
  void msm_task(JobCore& c, MsmRole role, const void* bases, const void* bases2, const void* scal, const MsmBatchArg* batch,
                size_t npts, const Fr* coef, size_t plen, hipStream_t stream, const MsmGate& gate, std::atomic<int>* raise,
                Then then, const MsmShare<Fr>* share = nullptr, std::atomic<int>* donated = nullptr) {
    JobCore* C = &c;
    const bool shared = share != nullptr;
    const MsmShare<Fr> sh = shared ? *share : MsmShare<Fr>{};
    const int dev = device;
    const bool batched = batch != nullptr;
    const MsmBatchArg ba = batched ? *batch : MsmBatchArg{};
    c.fut.push_back(pool_->submit([=]() {
      (void)hipSetDevice(dev);
      MsmPending* pend = &C->msm[role];
      int rc2 = msm_.template launch_t<Fld>(this, C->ws0 + role, bases, scal, npts, coef, plen, stream, pend, bases2, gate,
                                            batched ? &ba : nullptr, shared ? &sh : nullptr);
      if (donated) donated->store(rc2 ? -1 : 1, std::memory_order_release);      // (the U launch may be waiting for it)
      if (raise) raise->store(1, std::memory_order_release);
      else if (rc2 && gate.sorted_cnt) gate.sorted_cnt->fetch_add(1, std::memory_order_release);
      XYZZ<Fld> res[2 * MSM_MAXB];
      if (!rc2) rc2 = msm_fold_batch<Fld>(this, *pend, res, bases2 ? 2 : 1);
      C->rc[role] = rc2;
      if (!rc2) then(res);
    }));
  }
  // what the folded points of the witness MSMs are to the job's proofs
  void take_V(JobCore& c, const P2* res) {
    for (int b = 0; b < nproofs(c); b++) terms(c, b).V0 = res[b];
  }
  void take_W(JobCore& c, const P1* res) {
    for (int b = 0; b < nproofs(c); b++) terms(c, b).W = res[b];
  }
  // S (and H, res[nb + b]) of every proof, then s*S and r*H off the tail of a full proof (prove.rs:229-235, linearity):
  // the proofs of a batch are spread over the pool, this task takes proof 0
  void take_SH(JobCore& c, const P1* res, bool with_h) {
    const int nb = nproofs(c);
    JobCore* C = &c;
    auto fin = [=](int b) {
      ProofTerms& t = terms(*C, b);
      const bool h = with_h && !t.r_zero;
      t.S = res[b];
      if (h) t.H = res[nb + b];
      if (!t.full) return;
      t.sS = host_scalar_mul<FrP, Fq_>(t.S, t.s);
      if (h) t.rH = host_scalar_mul<FrP, Fq_>(t.H, t.r);
    };
    std::vector<std::future<void>> sub;
    for (int b = 1; b < nb; b++) sub.push_back(pool_->submit([=]() { fin(b); }));
    fin(0);
    // (the sub-tasks reference the caller's frame: the task runs queued work while it waits, HostPool::wait_helping -- a
    // pool whose workers all sit here with their sub-tasks queued behind them cannot starve)
    for (auto& f : sub)
      while (!pool_->wait_helping(f, deadline_from_now())) {}
  }

  // Starts one proof (full = all n parties and the assembly; otherwise the five partial d_msm sums of parties
  // [first, first + count) for the multi-GPU flow, where circom_h is driven by the caller and h arrives in finish).
  // A failure after the job has been marked active has aborted the job when this returns (bail): callers only return.
  int prove_begin(ProveJob& j, const zk_crs_share* crs, const void* qa, const void* qb, const void* qc,
                  const void* a_share, const void* ax_share, const Fr& r, const Fr& s, int log_m,
                  const zk_groth16_masks* mk, uint64_t seed, bool full, int first, int count, hipStream_t st,
                  bool gate_sorts = false, const HReport* report = nullptr) {
    if (j.active) return fail(ZK_ERR_BAD_INPUT, "a proof is already in flight on this slot");
    j.sharded = false;
    int rc = prove_begin_impl(j, crs, qa, qb, qc, a_share, ax_share, r, s, log_m, mk, seed, full, first, count, st,
                              gate_sorts, report);
    return rc && j.active ? bail(j, rc) : rc;
  }
  // the gate of a proof's U-MSM: its sort is event 3 of the "all sorts first" barrier (prove_begin_impl)
  MsmGate u_gate(ProveJob& j) {
    MsmGate g{};
    if (j.gate_sorts) {
      g.sorted_ev = j.ev_role[ROLE_U];
      g.sorted_cnt = &j.sorted_cnt;
    }
    return g;
  }
  int prove_begin_impl(ProveJob& j, const zk_crs_share* crs, const void* qa, const void* qb, const void* qc,
                       const void* a_share, const void* ax_share, const Fr& r, const Fr& s, int log_m,
                       const zk_groth16_masks* mk, uint64_t seed, bool full, int first, int count, hipStream_t st,
                       bool gate_sorts, const HReport* report = nullptr) {
    if (!Cfg::HAS_G2) return fail(ZK_ERR_BAD_INPUT, "G2 is not available for this curve");
    auto t_mark = std::chrono::steady_clock::now();
    auto host_span = [&](int slot) {                 // host:launch.* (zk_profile_read)
      if (!prof.on) return;
      const auto now = std::chrono::steady_clock::now();
      prof.host_add(slot, std::chrono::duration<double, std::milli>(now - t_mark).count());
      t_mark = now;
    };
    int rc = ensure_streams();
    if (!rc) rc = ensure_events(j);
    if (rc) return rc;
    init_terms(j.pt, crs, mk, r, s, full, first, count);
    for (int& e : j.rc) e = 0;
    const size_t Lc = ((size_t)1 << log_m) / l;
    // every internal stream is ordered after the work already queued on the caller's stream (the shares may still
    // be in flight there: found by tools/c5_bls381.py, where the a_share pack kernel of a 2^22 witness was still
    // running when the S/H/V MSMs started reading it)
    // (nothing to order after when the caller's stream has drained -- the case between two proofs of a loop: one query
    // instead of an event and six waits at the head of every chain of the proof)
    if (hipStreamQuery(st) != hipSuccess) {
      (void)hipGetLastError();                       // hipErrorNotReady is not an error here
      ZK_HIP(hipEventRecord(j.ev_in, st));
      for (hipStream_t is : streams_) ZK_HIP(hipStreamWaitEvent(is, j.ev_in, 0));
    }
    j.active = true;
    ProveJob* J = &j;
    const size_t cstride = crs->len_a;
    // ---- device pipelines: the four MSMs over the witness shares do not depend on h.  Each is enqueued by a pool task
    // (msm_task), which then waits for the slot's event and folds the windows on the host.
    // V (G2) is the longest chain: issued first, on a high-priority stream, as ONE launch over all parties (two halves
    // on two streams paid a second bucket reduction: 257 vs 279 proofs/s, round 2).
    // Orders that were measured and dropped (rounds 2-4, DESIGN.md "What bounds one proof"): V's accumulate ahead of the
    // G1 accumulates (283-285 vs 291-293 proofs/s), circom_h's launches enqueued ahead of the MSM tasks at the SHA-256
    // size (550-555 vs 571-596), S and H as two MSMs with their own sorts (391 vs 464), raised issue priority or shorter
    // lane ranges for the U-MSM (541-544 vs 591-594).
    const Fr* cf = msm_.coef_d_ + first;
    const Fr* cu = msm_.coef_d_;
    // a party list (zk_groth16_prove_checked_parties): the five MSM rounds and the host in-mask terms take the list's
    // coefficients, zero at the absent party -- a per-job vector in place of the tables; every launch keeps its shape, and
    // the bucket-sharing coefficients r * coef_p follow from it (MsmShare::scale1 multiplies what the launch is given)
    const bool listed = report && report->np > 0 && report->np < n;
    if (listed) {
      if (!full || first != 0 || count != n) return fail(ZK_ERR_BAD_INPUT, "a party list needs the full proof");
      std::vector<Fr> c;
      if ((rc = coefs_for(report->ids, report->np, c))) return rc;
      j.pt.coef.assign(n, Fr::zero());
      for (int i = 0; i < report->np; i++) j.pt.coef[report->ids[i]] = c[i];
      ZK_HIP(j.coef_d.ensure((size_t)n * sizeof(Fr)));
      ZK_HIP(hipMemcpy(j.coef_d.p, j.pt.coef.data(), (size_t)n * sizeof(Fr), hipMemcpyHostToDevice));
      cf = cu = (const Fr*)j.coef_d.p;
    }
    MsmGate gate{};
    // Large domains (2^h_first_log_m_ and up; 2^20 by default): circom_h and the SORT of the U-MSM that consumes it go
    // first, and the accumulate kernels of the witness MSMs wait for them (they still sort beside circom_h).  A proof of
    // this size is bound by the multiplier throughput of its five accumulate kernels whichever order they run in (0.667
    // vs 0.666 s per proof at 2^22, round 3), but next to four multi-hundred-millisecond accumulates every NTT pass (a
    // 512-thread / 64 KB workgroup needs a whole CU to drain) and every one-workgroup-per-CU sort kernel sat in the
    // dispatcher for most of the proof: the HIP-event spans of those slots then measured the wait, not the kernel
    // (0.43 s per sort against 25 ms of execution, profiles/r04_c5_kernel_stats.csv).
    // The witness MSMs also wait for EACH OTHER's sorts (V's accumulate alone holds every CU for 0.46 s at 2^24): every
    // launch of the proof records an event after its sort and counts itself in; an accumulate kernel is enqueued once all
    // four are on record, behind all four events.  The sharded prover (full == false) does the same: there the U sort is
    // enqueued by prove_launch_u once the king rounds of circom_h have been.
    const bool gated = j.gate_sorts = (full || gate_sorts) && log_m >= h_first_log_m_;
    j.sorted_cnt.store(0, std::memory_order_relaxed);
    if (gated) {
      gate.sorted_cnt = &j.sorted_cnt;
      gate.wait_sorted = j.ev_role;
      gate.n_wait_sorted = gate.sorted_need = 4;
    }
    auto role_gate = [&](MsmRole role) {
      MsmGate g = gate;
      if (g.n_wait_sorted) g.sorted_ev = J->ev_role[role];
      return g;
    };
    // report (zk_groth16_prove_checked): the checked h chain on the same stream with the same work buffers, its report into
    // the caller's buffers -- complete once the job's join has waited for the U chain; nothing else of the proof differs
    auto h_run = [&](hipStream_t hs) {
      return h_chain(HChain{1, &qa, &qb, &qc, log_m, mk, seed, (Fr*)J->hshare.p, report, &J->hwork, hs});
    };
    // ---- one bucket set for C.  C needs r*H + W + U only as a sum, and bucket accumulation is linear: where the launches
    // of H (the second vector of the S+H launch), W and U have the same bucket geometry -- with the registered SHA-256 CRS
    // all three use one set of 2^14 buckets -- H runs with r * coef_p as its coefficients, H and W stop behind their
    // finalize kernels and U's finalize kernel adds their buckets to its own (msm.hpp "SHARED BUCKET SET"): three bucket
    // sets are reduced and folded per proof instead of five and r*H costs no host multiplication.  Each of H and W shares
    // when ITS geometry equals U's (a table on one vector only, other "msm_table_c", table-free vectors of other lengths:
    // that launch is reduced on its own as before).  Not with the "all sorts first" order of large domains, where U is
    // enqueued ahead of the witness launches it would have to wait for on the host.
    const void* hd = j.pt.r_zero ? nullptr : crs->h_d;
    bool don_h = false, don_w = false;
    if (full && !gated) {
      MsmGeo gu, gd;
      if (msm_.template geometry<Fq_>(crs->u_d, nullptr, (size_t)n * crs->len_u, &gu)) {
        don_h = hd && msm_.template geometry<Fq_>(crs->s_d, hd, (size_t)count * cstride, &gd) && gd == gu;
        don_w = msm_.template geometry<Fq_>(crs->w_d, nullptr, (size_t)count * crs->len_w, &gd) && gd == gu;
      }
    }
    for (auto& f : j.don_flag) f.store(0, std::memory_order_relaxed);
    MsmShare<Fr> sh_h, sh_w, sh_u;
    if (don_h) {
      sh_h.keep = 1, sh_h.donated_ev = j.ev_don;
      sh_h.scale1_on = true, sh_h.scale1 = r;
      sh_u.from[sh_u.n_absorb] = &j.msm[ROLE_SH], sh_u.from_vec[sh_u.n_absorb] = 1, sh_u.from_flag[sh_u.n_absorb++] = &j.don_flag[0];
    }
    if (don_w) {
      sh_w.keep = 0;
      sh_u.from[sh_u.n_absorb] = &j.msm[ROLE_W], sh_u.from_vec[sh_u.n_absorb] = 0, sh_u.from_flag[sh_u.n_absorb++] = &j.don_flag[1];
    }
    bool hu_done = false;
    if (full && gated) {
      hipError_t he = j.hshare.ensure((size_t)n * Lc * sizeof(Fr));
      if (he != hipSuccess) return hip_fail(he, "h share buffer");
      rc = h_run(streams_[5]);
      if (rc) return rc;
      rc = msm_.template launch_t<Fq_>(this, j.ws0 + ROLE_U, crs->u_d, j.hshare.p, (size_t)n * crs->len_u,
                                      cu, crs->len_u, streams_[5], &j.msm[ROLE_U], nullptr, u_gate(j));
      if (rc) return rc;
      hu_done = true;
    }
    msm_task<Fq2_>(j, ROLE_V, crs->v_d, nullptr, a_share, nullptr, (size_t)count * cstride, cf, cstride, streams_[2],
                   role_gate(ROLE_V), nullptr, [this, J](const P2* res) { take_V(*J, res); });
    // S and H multiply two base vectors by the same witness shares: ONE launch over both vectors, each with its own sort
    // (their identity bases differ: b_query is the identity for every wire no B-row mentions, 59 % in the SHA-256 circuit)
    const bool fold_h = hd != nullptr && !don_h;
    msm_task<Fq_>(j, ROLE_SH, crs->s_d, hd, a_share, nullptr, (size_t)count * cstride, cf, cstride, streams_[0],
                  role_gate(ROLE_SH), nullptr, [this, J, fold_h](const P1* res) { take_SH(*J, res, fold_h); },
                  don_h ? &sh_h : nullptr, don_h ? &j.don_flag[0] : nullptr);
    msm_task<Fq_>(j, ROLE_W, crs->w_d, nullptr, ax_share, nullptr, (size_t)count * crs->len_w, cf, crs->len_w, streams_[3],
                  role_gate(ROLE_W), nullptr, [this, J](const P1* res) { take_W(*J, res); },
                  don_w ? &sh_w : nullptr, don_w ? &j.don_flag[1] : nullptr);
    // (the host terms are two dozen pool submissions: behind circom_h's launches when those are still to come -- they
    // are the head of the proof's longest chain and the terms are not needed before prove_end)
    if (!(full && !hu_done)) submit_host_terms(&j.pt, j.fut);
    // ---- circom_h and the U-MSM that depends on it form a long dependent chain: high-priority internal stream.
    // At the SHA-256 size, holding the other MSM streams (or only their accumulate launches) back until circom_h has
    // finished was measured and rejected: 8.6-8.8 ms per proof against 6.9 ms when everything is issued at once.
    if (full && !hu_done) {
      host_span(PROF_HOST_SUBMIT);
      hipStream_t hs = streams_[5];
      hipError_t he = j.hshare.ensure((size_t)n * Lc * sizeof(Fr));
      if (he != hipSuccess) return hip_fail(he, "h share buffer");
      rc = h_run(hs);
      if (rc) return rc;
      host_span(PROF_HOST_H);
      rc = msm_.template launch_t<Fq_>(this, j.ws0 + ROLE_U, crs->u_d, j.hshare.p, (size_t)n * crs->len_u,
                                      cu, crs->len_u, hs, &j.msm[ROLE_U], nullptr, MsmGate{}, nullptr,
                                      sh_u.n_absorb ? &sh_u : nullptr);
      if (rc) return rc;
      submit_host_terms(&j.pt, j.fut);
      host_span(PROF_HOST_U);
    }
    return ZK_OK;
  }

  // Host-side terms of one proof that depend on nothing but its inputs (scalar multiples of CRS constants, in-mask sums,
  // per-party multiples of the out-masks): tasks of the worker pool, running beside the device work.
  void submit_host_terms(ProofTerms* J, std::vector<std::future<void>>& fut) {
    const bool full = J->full;
    const int first = J->first, count = J->count;
    if (full) {
      fut.push_back(pool_->submit([J]() {
        P1 d1 = aff1(J->crs.delta_g1);
        J->rN = host_scalar_mul<FrP, Fq_>(d1, J->r);
        J->s_cA = host_scalar_mul<FrP, Fq_>(xyzz_add_ni(xyzz_add_ni(aff1(J->crs.a_query0), J->rN), aff1(J->crs.alpha_g1)), J->s);
      }));
      fut.push_back(pool_->submit([J]() {
        P1 d1 = aff1(J->crs.delta_g1);
        J->sK = host_scalar_mul<FrP, Fq_>(d1, J->s);
        J->r_cB1 = host_scalar_mul<FrP, Fq_>(xyzz_add_ni(xyzz_add_ni(aff1(J->crs.b_g1_query0), J->sK), aff1(J->crs.beta_g1)), J->r);
      }));
      fut.push_back(pool_->submit([J]() { J->rsM = host_scalar_mul<FrP, Fq_>(aff1(J->crs.delta_g1), J->r * J->s); }));
      fut.push_back(pool_->submit([J]() { J->sK2 = host_scalar_mul<FrP, Fq2_>(aff2(J->crs.delta_g2), J->s); }));
    }
    const zk_groth16_masks* mk = J->masks();
    if (mk) {
      // in-mask terms sum_p coef_p * mask_p (the king's unpack2 + sum over the masked points, dmsm/mod.rs:85-86)
      for (int k = 0; k < 5; k++) {
        if (!mk->msm_in[k] || (k == 1 && J->r_zero)) continue;
        const void* im = mk->msm_in[k];
        fut.push_back(pool_->submit([this, J, k, im, first, count]() {
          if (k == 2) {
            J->in2 = msm_.template mask_term<Fq2_>(im, first, count, J->coefs());
          } else {
            J->in1[k] = msm_.template mask_term<Fq_>(im, first, count, J->coefs());
            if (k == 0 && J->full) J->s_in0 = host_scalar_mul<FrP, Fq_>(J->in1[0], J->s);
            if (k == 1 && J->full) J->r_in1 = host_scalar_mul<FrP, Fq_>(J->in1[1], J->r);
          }
        }));
      }
      // per-party multiples of the out-masks of A and B1 that enter C = s*A + r*B1 + ...
      if (full)
        for (int p = 0; p < n; p++) {
          if (mk->msm_out[0])
            fut.push_back(pool_->submit([J, p]() {
              J->s_om0[p] = host_scalar_mul<FrP, Fq_>(jacobian_to_xyzz(((const Jacobian<Fq_>*)J->mk.msm_out[0])[p]), J->s);
            }));
          if (mk->msm_out[1] && !J->r_zero)
            fut.push_back(pool_->submit([J, p]() {
              J->r_om1[p] = host_scalar_mul<FrP, Fq_>(jacobian_to_xyzz(((const Jacobian<Fq_>*)J->mk.msm_out[1])[p]), J->r);
            }));
        }
    }
  }

  // the U-MSM of a partial job (h comes from the caller's king rounds)
  int prove_launch_u(ProveJob& j, const void* h_share, hipStream_t st) {
    const ProofTerms& t = j.pt;
    return msm_.template launch_t<Fq_>(this, j.ws0 + ROLE_U, t.crs.u_d, h_share, (size_t)t.count * t.crs.len_u,
                                      msm_.coef_d_ + t.first, t.crs.len_u, st, &j.msm[ROLE_U], nullptr, u_gate(j));
  }

  // The end of one proof.  The U chain (circom_h, then its MSM) ends last by a margin: everything that does not depend on U
  // -- the join of the pool tasks, A and B of every party, C without its U term -- is done while it still runs; after U's
  // event only its fold (join) and one addition per party are left.
  int prove_end(ProveJob& j, void* pi_a, void* pi_b, void* pi_c) {
    const char* who = "zk_groth16_wait";
    const auto t0 = std::chrono::steady_clock::now();
    int rc = drain_or_wedge(j, who);
    if (rc) return rc;
    bool early_ok = !j.pt.err.code;
    for (int e : j.rc) early_ok = early_ok && !e;
    std::vector<P1> c_part(early_ok ? n : 0);
    if (early_ok) assemble_job(j.pt, j.pt.sums(), pi_a, pi_b, pi_c, c_part.data());    // (U is still the identity there)
    if (prof.on && job_slot(j, ROLE_U).busy) (void)event_wait(job_slot(j, ROLE_U).ev);   // (the join waits again: returns at once)
    const auto t2 = std::chrono::steady_clock::now();
    struct HostSpans {                                                          // host:prove_wait / host:prove_tail
      Profiler& pr;
      std::chrono::steady_clock::time_point a, b;
      ~HostSpans() {
        if (!pr.on) return;
        pr.host_add(PROF_HOST_WAIT, std::chrono::duration<double, std::milli>(b - a).count());
        pr.host_add(PROF_HOST_TAIL, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b).count());
      }
    } spans{prof, t0, t2};
    rc = join(j, who);              // (a failed task or term, the reason for !early_ok, is returned here)
    if (rc) return rc;
    Jacobian<Fq_>* oc = (Jacobian<Fq_>*)pi_c;
    for (int p = 0; p < n; p++) oc[p] = xyzz_to_jacobian(xyzz_add_ni(c_part[p], j.pt.U));
    return ZK_OK;
  }
  // the n parties' (A, B, C) shares of one proof from its five MSM totals (in-mask terms included) and the host terms
  // (c_part != nullptr: the C shares stay in extended form there instead of pi_c -- prove_end adds a late term to them)
  void assemble_job(const ProofTerms& j, const MsmSums& t, void* pi_a, void* pi_b, void* pi_c, P1* c_part = nullptr) {
    const zk_groth16_masks* mk = j.masks();
    // prove.rs:40-56 / 99-110 / 148-158 / 229-235 for every party; C = s*A + r*B1 - rs*delta + W + U by linearity:
    //   s*A_p = s*(a0 + r*delta + alpha) + s*S + s*in0 + s*om0_p     (every term was computed beside the device work;
    //   r*B1_p likewise, so the total H itself is not needed)
    P1 cA = xyzz_add_ni(xyzz_add_ni(aff1(j.crs.a_query0), j.rN), aff1(j.crs.alpha_g1));
    P2 cB2 = xyzz_add_ni(xyzz_add_ni(aff2(j.crs.b_g2_query0), j.sK2), aff2(j.crs.beta_g2));
    P1 A0 = xyzz_add_ni(cA, t.S);
    P2 B0 = xyzz_add_ni(cB2, t.V);
    P1 C0 = xyzz_add_ni(xyzz_add_ni(j.s_cA, j.sS), j.s_in0);
    if (!j.r_zero) C0 = xyzz_add_ni(C0, xyzz_add_ni(xyzz_add_ni(j.r_cB1, j.rH), j.r_in1));
    C0 = xyzz_add_ni(C0, j.rsM.neg());
    C0 = xyzz_add_ni(C0, xyzz_add_ni(t.W, t.U));
    Jacobian<Fq_>* oa = (Jacobian<Fq_>*)pi_a;
    Jacobian<Fq2_>* ob = (Jacobian<Fq2_>*)pi_b;
    Jacobian<Fq_>* oc = (Jacobian<Fq_>*)pi_c;
    auto om1 = [&](int k, int p) { return jacobian_to_xyzz(((const Jacobian<Fq_>*)mk->msm_out[k])[p]); };
    const bool uniform = !mk || (!mk->msm_out[0] && !mk->msm_out[1] && !mk->msm_out[2] && !mk->msm_out[3] &&
                                 !mk->msm_out[4]);
    for (int p = 0; p < n; p++) {
      if (uniform && p > 0) {
        oa[p] = oa[0];
        ob[p] = ob[0];
        if (c_part) c_part[p] = c_part[0];
        else oc[p] = oc[0];
        continue;
      }
      P1 A = A0, C = C0;
      P2 B2 = B0;
      if (!uniform) {
        if (mk->msm_out[0]) {
          A = xyzz_add_ni(A, om1(0, p));
          C = xyzz_add_ni(C, j.s_om0[p]);
        }
        if (mk->msm_out[1] && !j.r_zero) C = xyzz_add_ni(C, j.r_om1[p]);
        if (mk->msm_out[2]) B2 = xyzz_add_ni(B2, jacobian_to_xyzz(((const Jacobian<Fq2_>*)mk->msm_out[2])[p]));
        if (mk->msm_out[3]) C = xyzz_add_ni(C, om1(3, p));
        if (mk->msm_out[4]) C = xyzz_add_ni(C, om1(4, p));
      }
      oa[p] = xyzz_to_jacobian(A);
      ob[p] = xyzz_to_jacobian(B2);
      if (c_part) c_part[p] = C;
      else oc[p] = xyzz_to_jacobian(C);
    }
  }

  int check_prove_args(const zk_crs_share* crs, const void* r_, const void* s_, int log_m) {
    if (!Cfg::HAS_G2) return fail(ZK_ERR_BAD_INPUT, "G2 is not available for this curve");
    int rc = check_wedged();
    if (rc) return rc;
    if (!crs || !r_ || !s_) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    int log_l = ilog2(l);
    if (log_m < log_l || log_m + 1 > FrP::TWO_ADICITY) return fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT");
    if (crs->len_u != ((size_t)1 << log_m) / l)
      return fail(ZK_ERR_BAD_INPUT, "h_query share length must be m/l");   // dmsm/mod.rs:71
    return ZK_OK;
  }

  int groth16_prove(const zk_crs_share* crs, const void* qa, const void* qb, const void* qc, const void* a_share,
                    const void* ax_share, const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk,
                    uint64_t seed, void* pi_a, void* pi_b, void* pi_c, hipStream_t st) override {
    if (!pi_a || !pi_b || !pi_c) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    int h = -1;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = groth16_prove_async(crs, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, st, &h);
    if (rc) return rc;
    if (prof.on) prof.host_add(PROF_HOST_LAUNCH, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return groth16_wait(h, pi_a, pi_b, pi_c);
  }
  // zk_groth16_prove_checked: the proof above with circom_h's seven king words checked (engine_h.inc.hpp h_chain with a report).  The five d_msm
  // rounds stay unchecked.  The asynchronous form followed by the join, which orders the report buffers.
  int groth16_prove_checked(const zk_crs_share* crs, const void* qa, const void* qb, const void* qc, const void* a_share,
                            const void* ax_share, const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk,
                            uint64_t seed, void* pi_a, void* pi_b, void* pi_c, uint8_t* status, uint32_t* errpos,
                            uint64_t* summary, hipStream_t st) override {
    if (!pi_a || !pi_b || !pi_c || !status) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    int h = -1;
    int rc = groth16_prove_checked_async(crs, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, status, errpos, summary,
                                         st, &h);
    if (rc) return rc;
    return groth16_wait(h, pi_a, pi_b, pi_c);
  }
  // zk_groth16_prove_checked_async: the report descriptor goes into the job (prove_start); zk_groth16_wait joins it like any
  // proof -- the h chain runs ahead of the U-MSM on the job's stream, so the report is complete when the join returns
  int groth16_prove_checked_async(const zk_crs_share* crs, const void* qa, const void* qb, const void* qc, const void* a_share,
                                  const void* ax_share, const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk,
                                  uint64_t seed, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st,
                                  int* handle) override {
    if (!status) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    const HReport report{status, errpos, summary};
    return prove_start(crs, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, st, handle, &report);
  }
  // zk_groth16_prove_checked_parties: the checked proof from the words and MSM contributions of a party list -- the h chain
  // of circom_h_checked_parties, the list's coefficients in the five MSM rounds and the host in-mask terms (prove_begin_impl)
  int groth16_prove_checked_parties(const uint32_t* parties, int np, const zk_crs_share* crs, const void* qa, const void* qb,
                                    const void* qc, const void* a_share, const void* ax_share, const void* r_, const void* s_,
                                    int log_m, const zk_groth16_masks* mk, uint64_t seed, void* pi_a, void* pi_b, void* pi_c,
                                    uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    uint32_t ids[GAO_MAX_N];
    int rc = checked_list(parties, np, 2 * l, ids);
    if (rc) return rc;
    if (!pi_a || !pi_b || !pi_c || !status) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    int h = -1;
    rc = groth16_prove_checked_parties_async(parties, np, crs, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, status,
                                             errpos, summary, st, &h);
    if (rc) return rc;
    return groth16_wait(h, pi_a, pi_b, pi_c);
  }
  // zk_groth16_prove_checked_parties_async: the list is validated here and copied into the job by prove_start; `parties` is
  // not read after the call returns
  int groth16_prove_checked_parties_async(const uint32_t* parties, int np, const zk_crs_share* crs, const void* qa,
                                          const void* qb, const void* qc, const void* a_share, const void* ax_share,
                                          const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk, uint64_t seed,
                                          uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st,
                                          int* handle) override {
    uint32_t ids[GAO_MAX_N];
    int rc = checked_list(parties, np, 2 * l, ids);
    if (rc) return rc;
    if (!status) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    HReport report{status, errpos, summary};
    if (np < n) report.ids = ids, report.np = np;
    return prove_start(crs, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, st, handle, &report);
  }
  int groth16_prove_async(const zk_crs_share* crs, const void* qa, const void* qb, const void* qc, const void* a_share,
                          const void* ax_share, const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk,
                          uint64_t seed, hipStream_t st, int* handle) override {
    return prove_start(crs, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, st, handle, nullptr);
  }
  int prove_start(const zk_crs_share* crs, const void* qa, const void* qb, const void* qc, const void* a_share,
                  const void* ax_share, const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk, uint64_t seed,
                  hipStream_t st, int* handle, const HReport* report) {
    int rc = check_prove_args(crs, r_, s_, log_m);
    if (rc) return rc;
    if (!qa || !qb || !qc || !a_share || !ax_share || !handle) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    ProveJob* j = free_job(jobs_);
    if (!j) return fail(ZK_ERR_BAD_INPUT, "too many proofs in flight (zk_groth16_wait one first)");
    Fr r = Fr::from_limbs((const uint32_t*)r_), s = Fr::from_limbs((const uint32_t*)s_);
    // the job's own copy of the report descriptor and of the list
    if ((j->checked = report != nullptr)) {
      j->report = *report;
      if (report->np > 0) {
        std::copy(report->ids, report->ids + report->np, j->report_ids);
        j->report.ids = j->report_ids;
      }
      report = &j->report;
    }
    rc = prove_begin(*j, crs, qa, qb, qc, a_share, ax_share, r, s, log_m, mk, seed, true, 0, n, st, false, report);
    if (rc) return rc;
    *handle = j->slot;
    return ZK_OK;
  }
  int groth16_wait(int handle, void* pi_a, void* pi_b, void* pi_c) override {
    if (handle < 0 || handle >= NJOBS || !jobs_[handle].active) return fail(ZK_ERR_BAD_INPUT, "no proof in flight on this handle");
    if (jobs_[handle].sharded) return fail(ZK_ERR_BAD_INPUT, "a sharded proof is in flight on this handle: zk_dist_groth16_wait joins it");
    if (!pi_a || !pi_b || !pi_c) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    return prove_end(jobs_[handle], pi_a, pi_b, pi_c);
  }
  // also the abort of a sharded proof in flight (zk_dist_groth16_prove_async hands out handles of the same space): the
  // slot is free for either kind afterwards.  The channels' round counters are NOT rewound -- every rank must abort the
  // same proof, as every rank must issue the same sequence of collective calls.
  int groth16_abort(int handle) override {
    if (handle < 0 || handle >= NJOBS) return fail(ZK_ERR_BAD_INPUT, "bad handle");
    abort(jobs_[handle]);
    jobs_[handle].sharded = false;
    return ZK_OK;
  }

  // ---------------------------------------------------------------- a batch of proofs against one CRS
  // zk_groth16_prove_batch: `nb` witnesses proved against the SAME packed CRS in one pass.  The reference runs its
  // parties as concurrent tasks and a service runs proofs concurrently (mpc-net/src/multi.rs:317-327,
  // groth16/examples/sha256.rs:316-360); one proof of the SHA-256 circuit leaves most of the chip idle (a dozen short
  // dependent launches per MSM, 2.3 waves per SIMD in the accumulate), so the batch goes through every stage TOGETHER:
  // each of the five MSMs is ONE sort / accumulate / finalize / reduce chain over nb scalar vectors against one base
  // vector (msm.hpp MsmScalars: bucket sets indexed by (proof, window)), circom_h is one launch chain over 3 nb
  // vectors.  Host terms (scalar multiples of masks and CRS constants) are per proof, on the worker pool as before.
  static constexpr int MAX_PROOF_BATCH = MSM_MAXB;

  int groth16_prove_batch(const zk_crs_share* crs, int nb, const void* const* qa, const void* const* qb,
                          const void* const* qc, const void* const* a_share, const void* const* ax_share, const void* r_,
                          const void* s_, int log_m, const zk_groth16_masks* mk, uint64_t seed, void* pi_a, void* pi_b,
                          void* pi_c, hipStream_t st) override {
    if (!pi_a || !pi_b || !pi_c) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    int h = -1;
    int rc = groth16_prove_batch_async(crs, nb, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, st, &h);
    if (rc) return rc;
    return groth16_batch_wait(h, pi_a, pi_b, pi_c);
  }
  int groth16_prove_batch_async(const zk_crs_share* crs_in, int nb, const void* const* qa, const void* const* qb,
                                const void* const* qc, const void* const* a_share, const void* const* ax_share,
                                const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk, uint64_t seed,
                                hipStream_t st, int* handle) override {
    return batch_start(crs_in, nb, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, st, handle, nullptr);
  }
  // zk_groth16_prove_checked_batch: the batch above on the checked h chain of a batch (h_chain with a report) with the
  // batch's own hwork, and so its own staging report; the five d_msm rounds stay unchecked as in the single call.  The
  // report (proof-major, [nb][7]) is complete when zk_groth16_batch_wait returns.
  int groth16_prove_checked_batch(const zk_crs_share* crs, int nb, const void* const* qa, const void* const* qb,
                                  const void* const* qc, const void* const* a_share, const void* const* ax_share,
                                  const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk, uint64_t seed,
                                  void* pi_a, void* pi_b, void* pi_c, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                                  hipStream_t st) override {
    if (!pi_a || !pi_b || !pi_c) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    int h = -1;
    int rc = groth16_prove_checked_batch_async(crs, nb, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, status, errpos,
                                               summary, st, &h);
    if (rc) return rc;
    return groth16_batch_wait(h, pi_a, pi_b, pi_c);
  }
  int groth16_prove_checked_batch_async(const zk_crs_share* crs, int nb, const void* const* qa, const void* const* qb,
                                        const void* const* qc, const void* const* a_share, const void* const* ax_share,
                                        const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk, uint64_t seed,
                                        uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st,
                                        int* handle) override {
    if (!status) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    const HReport report{status, errpos, summary};
    return batch_start(crs, nb, qa, qb, qc, a_share, ax_share, r_, s_, log_m, mk, seed, st, handle, &report);
  }
  int batch_start(const zk_crs_share* crs_in, int nb, const void* const* qa, const void* const* qb, const void* const* qc,
                  const void* const* a_share, const void* const* ax_share, const void* r_, const void* s_, int log_m,
                  const zk_groth16_masks* mk, uint64_t seed, hipStream_t st, int* handle, const HReport* report) {
    if (!qa || !qb || !qc || !handle) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (nb >= 1 && nb <= MAX_PROOF_BATCH)
      for (int b = 0; b < nb; b++)
        if (!qa[b] || !qb[b] || !qc[b]) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    BatchJob* B = nullptr;
    int rc = batch_begin(crs_in, nb, a_share, ax_share, r_, s_, log_m, mk, true, 0, n, st, &B);
    if (rc) return rc;
    // ---- circom_h of the whole batch and the U-MSM behind it
    const size_t Lc = ((size_t)1 << log_m) / l, per = (size_t)n * Lc;
    rc = h_chain(HChain{nb, qa, qb, qc, log_m, mk, seed, (Fr*)B->hshare.p, report, &B->hwork, B->st[5]});
    if (!rc) rc = batch_launch_u(*B, (const Fr*)B->hshare.p, per, B->st[5]);
    if (rc) return bail(*B, rc);
    *handle = B->slot;
    return ZK_OK;
  }
  // the U-MSM of a batch: h_all = [nb][count * m/l] (proof b at h_all + b * stride)
  int batch_launch_u(BatchJob& B, const Fr* h_all, size_t stride, hipStream_t st) {
    const ProofTerms& t = B.pt[0];                   // (CRS and party range are the batch's)
    MsmBatchArg ba_h;
    ba_h.nb = B.nb;
    for (int b = 0; b < B.nb; b++) ba_h.p[b] = h_all + (size_t)b * stride;
    int rc = msm_.template launch_t<Fq_>(this, B.ws0 + ROLE_U, t.crs.u_d, nullptr, (size_t)t.count * t.crs.len_u,
                                        msm_.coef_d_ + t.first, t.crs.len_u, st, &B.msm[ROLE_U], nullptr, B.gate_u, &ba_h);
    B.acc_flag[ROLE_U].store(1, std::memory_order_release);
    return rc;
  }
  // Starts a batch: the four witness MSMs of parties [first, first + count) for nb proofs (one launch chain each) and
  // the proofs' host terms.  full: all n parties, assembly included; otherwise the partial sums of one rank (the in-mask
  // terms only).  The caller enqueues circom_h and batch_launch_u, then joins.
  int batch_begin(const zk_crs_share* crs, int nb, const void* const* a_share, const void* const* ax_share,
                  const void* r_, const void* s_, int log_m, const zk_groth16_masks* mk, bool full, int first, int count,
                  hipStream_t st, BatchJob** job_out) {
    if (!Cfg::HAS_G2) return fail(ZK_ERR_BAD_INPUT, "G2 is not available for this curve");
    int rc = check_prove_args(crs, r_, s_, log_m);
    if (rc) return rc;
    if (nb < 1 || nb > MAX_PROOF_BATCH || 3 * nb > KING_BATCH || nb > DEGRED_BATCH)
      return fail(ZK_ERR_BAD_INPUT, "batch size must be in 1.." + std::to_string(MAX_PROOF_BATCH));
    if (!a_share || !ax_share) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    for (int b = 0; b < nb; b++)
      if (!a_share[b] || !ax_share[b]) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    BatchJob* Bp = free_job(bjobs_);
    if (!Bp) return fail(ZK_ERR_BAD_INPUT, "too many batches in flight (zk_groth16_batch_wait one first)");
    BatchJob& B = *Bp;
    rc = ensure_streams();
    if (!rc) rc = ensure_events(B);
    if (rc) return rc;
    // (splitting the chip between the G2 MSM and the rest with CU masks was measured in round 3 and dropped: DESIGN.md
    // "batched proving")
    B.own_streams = B.slot != 0;
    for (int i = 0; i < 6; i++) {
      if (B.st[i]) continue;
      if (!B.own_streams) {
        B.st[i] = streams_[i];                       // batch slot 0 shares the single-proof stream set
      } else {
        int pr = 0;
        ZK_HIP(hipStreamGetPriority(streams_[i], &pr));
        ZK_HIP(hipStreamCreateWithPriority(&B.st[i], hipStreamNonBlocking, pr));
      }
    }
    const size_t Lc = ((size_t)1 << log_m) / l, per = (size_t)count * Lc;
    ZK_HIP(B.hshare.ensure(per * nb * sizeof(Fr)));
    B.nb = nb;
    while ((int)B.pt.size() < nb) B.pt.emplace_back();
    bool all_r_zero = true;
    for (int b = 0; b < nb; b++) {
      Fr r = Fr::from_limbs((const uint32_t*)r_ + (size_t)b * FrP::N), s = Fr::from_limbs((const uint32_t*)s_ + (size_t)b * FrP::N);
      init_terms(B.pt[b], crs, mk ? &mk[b] : nullptr, r, s, full, first, count);
      all_r_zero = all_r_zero && r.is_zero();
    }
    for (int& e : B.rc) e = 0;
    ZK_HIP(hipEventRecord(B.ev_in, st));
    for (int i = 0; i < 6; i++) ZK_HIP(hipStreamWaitEvent(B.st[i], B.ev_in, 0));
    B.active = true;
    const Fr* cf = msm_.coef_d_ + first;
    MsmBatchArg ba_a, ba_x;
    ba_a.nb = ba_x.nb = nb;
    for (int b = 0; b < nb; b++) {
      ba_a.p[b] = a_share[b];
      ba_x.p[b] = ax_share[b];
    }
    // Order of the accumulate kernels.  Each accumulate of a batch fills the chip by itself (two or more rounds of
    // waves), so running them ONE AFTER THE OTHER loses nothing -- the sorts, finalizes and reductions of the other MSMs
    // run beside it -- and spares them each other: issued together, four kernels' waves interleave on every SIMD, the
    // 256-register G2 waves are crowded out by the 168-register G1 waves (which fit any slot a G1 wave frees) and V's
    // accumulate ends alone long after the others with its reduction tail on an empty chip
    // (profiles/r03_b8_timeline_*.txt).  The chain in order, by the first letters of ROLE_NAME (S = the S + H launch);
    // "-" = no chain.  (A small batch does not fill the chip with one accumulate: its kernels run side by side as in a
    // single proof.)
    const std::string order = nb >= 4 ? "VSWU" : "-";
    MsmGate gates[NROLES];
    {
      int prev = -1;
      for (char ch : order) {
        int id = -1;
        for (int r = 0; r < NROLES; r++)
          if (ROLE_NAME[r][0] == ch) id = r;
        if (id < 0 || gates[id].signal_ev) continue;
        B.acc_flag[id].store(0, std::memory_order_relaxed);
        gates[id].signal_ev = B.ev_role[id];
        gates[id].signal_flag = &B.acc_flag[id];
        if (prev >= 0) {
          gates[id].wait_ev = B.ev_role[prev];
          gates[id].wait_flag = &B.acc_flag[prev];
        }
        prev = id;
      }
    }
    // ---- the witness MSMs: V (G2) first on its high-priority stream, S + H as one launch over both base vectors, W
    msm_task<Fq2_>(B, ROLE_V, crs->v_d, nullptr, nullptr, &ba_a, (size_t)count * crs->len_a, cf, crs->len_a, B.st[2],
                   gates[ROLE_V], &B.acc_flag[ROLE_V], [this, Bp](const P2* res) { take_V(*Bp, res); });
    const void* hd = all_r_zero ? nullptr : crs->h_d;
    msm_task<Fq_>(B, ROLE_SH, crs->s_d, hd, nullptr, &ba_a, (size_t)count * crs->len_a, cf, crs->len_a, B.st[0],
                  gates[ROLE_SH], &B.acc_flag[ROLE_SH], [this, Bp, hd](const P1* res) { take_SH(*Bp, res, hd != nullptr); });
    msm_task<Fq_>(B, ROLE_W, crs->w_d, nullptr, nullptr, &ba_x, (size_t)count * crs->len_w, cf, crs->len_w, B.st[3],
                  gates[ROLE_W], &B.acc_flag[ROLE_W], [this, Bp](const P1* res) { take_W(*Bp, res); });
    // ---- host terms of every proof
    for (int b = 0; b < nb; b++) submit_host_terms(&B.pt[b], B.fut);
    B.gate_u = gates[ROLE_U];
    *job_out = Bp;
    return ZK_OK;
  }
  int groth16_batch_wait(int handle, void* pi_a, void* pi_b, void* pi_c) override {
    if (handle < 0 || handle >= NBATCH || !bjobs_[handle].active) return fail(ZK_ERR_BAD_INPUT, "no batch in flight on this handle");
    BatchJob& B = bjobs_[handle];
    if (!pi_a || !pi_b || !pi_c) {
      abort(B);
      return fail(ZK_ERR_BAD_INPUT, "null pointer");
    }
    int rc = join(B, "zk_groth16_batch_wait");
    if (rc) return rc;
    for (int b = 0; b < B.nb; b++)
      assemble_job(B.pt[b], B.pt[b].sums(), (char*)pi_a + (size_t)b * n * sizeof(Jacobian<Fq_>),
                   (char*)pi_b + (size_t)b * n * sizeof(Jacobian<Fq2_>), (char*)pi_c + (size_t)b * n * sizeof(Jacobian<Fq_>));
    return ZK_OK;
  }

  // zk_msm_batch: G::msm of ONE base vector against `nb` scalar vectors (the sort / accumulate / reduce chain of
  // msm.hpp runs once for the batch); out: nb Jacobian points (host).
  int msm_batch(int group, const void* bases, size_t len, const void* const* scalars, int nb, void* out,
                hipStream_t st) override {
    if (nb < 1 || nb > MSM_MAXB) return fail(ZK_ERR_BAD_INPUT, "batch size must be in 1.." + std::to_string(MSM_MAXB));
    if (!out || !scalars || (len && !bases)) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    MsmBatchArg ba;
    ba.nb = nb;
    for (int b = 0; b < nb; b++) {
      if (len && !scalars[b]) return fail(ZK_ERR_BAD_INPUT, "null pointer");
      ba.p[b] = scalars[b];
    }
    return msm_.by_group(this, group, [&](auto fld) -> int {
      using Fld = decltype(fld);
      std::vector<XYZZ<Fld>> res((size_t)nb);
      int rc = msm_.run_t(this, -1, bases, nullptr, len, nullptr, 1, st, res.data(), [] {}, &ba);
      if (rc) return rc;
      for (int b = 0; b < nb; b++) msm_.write_jacobian((char*)out + (size_t)b * sizeof(Jacobian<Fld>), res[b]);
      return ZK_OK;
    });
  }

  // sum over the listed local parties of coef_p * (msm_p + in_mask_p): one rank's contribution to the king's
  // unpack2 + sum (dmsm/mod.rs:85-86) when the n parties are spread over several GPUs.
  int d_msm_local(int group, const void* bases, const void* scalars, size_t len, int first_party, int nparties,
                  const void* in_mask, void* out, hipStream_t st) override {
    if (first_party < 0 || nparties <= 0 || first_party + nparties > n) return fail(ZK_ERR_BAD_INPUT, "bad party range");
    if (!out) return fail(ZK_ERR_BAD_INPUT, "null output");
    return msm_.by_group(this, group, [&](auto fld) {
      XYZZ<decltype(fld)> r;
      int rc = msm_.d_msm_range_t(this, bases, scalars, len, first_party, nparties, in_mask, &r, st);
      if (!rc) msm_.write_jacobian(out, r);
      return rc;
    });
  }
  // MsmMask::sample (dmsm/mod.rs:21-47); scalar form: shares of (x_0..x_{l-1} | t random) times the generator
  template <class Fld>
  int msm_mask_sample_t(const void* gen_affine, uint64_t seed, void* in_mask, void* out_mask) {
    Affine<Fld> g;
    memcpy(&g, gen_affine, sizeof(g));
    XYZZ<Fld> gen = XYZZ<Fld>::from_affine(g);
    const int k = l + t;
    std::vector<Fr> sec_in(k), sec_out(k);
    Fr sum = Fr::zero();
    const RngSeed r0 = rs_host(seed), r1 = rs_host(seed ^ 0x1111ull), r2 = rs_host(seed ^ 0x2222ull);
    for (int i = 0; i < l; i++) {
      sec_in[i] = rand_fp<FrP>(r0, (uint64_t)i);
      sum = sum + sec_in[i];
    }
    for (int i = 0; i < l; i++) sec_out[i] = sum.neg();
    for (int i = 0; i < t; i++) {
      sec_in[l + i] = rand_fp<FrP>(r1, (uint64_t)i);
      sec_out[l + i] = rand_fp<FrP>(r2, (uint64_t)i);
    }
    Jacobian<Fld>* oi = (Jacobian<Fld>*)in_mask;
    Jacobian<Fld>* oo = (Jacobian<Fld>*)out_mask;
    for (int p = 0; p < n; p++) {
      Fr si = Fr::zero(), so = Fr::zero();
      for (int j = 0; j < k; j++) {
        si = si + pmat_host_[(size_t)p * k + j] * sec_in[j];
        so = so + pmat_host_[(size_t)p * k + j] * sec_out[j];
      }
      oi[p] = xyzz_to_jacobian(host_scalar_mul<FrP, Fld>(gen, si));
      oo[p] = xyzz_to_jacobian(host_scalar_mul<FrP, Fld>(gen, so));
    }
    return ZK_OK;
  }
  int msm_mask_sample(int group, const void* gen_affine, uint64_t seed, void* in_mask, void* out_mask) override {
    using Fq = Fp<typename Cfg::FqP>;
    using Fq2 = Fp2<typename Cfg::FqP>;
    if (!gen_affine || !in_mask || !out_mask) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (group == ZK_G1) return msm_mask_sample_t<Fq>(gen_affine, seed, in_mask, out_mask);
    if (group == ZK_G2 && Cfg::HAS_G2) return msm_mask_sample_t<Fq2>(gen_affine, seed, in_mask, out_mask);
    return fail(ZK_ERR_BAD_INPUT, "bad group");
  }

  // ---------------------------------------------------------------- zk_groth16_deal_masks
  // All twelve masks of `nproofs` proofs (sha256.rs:226-291), in passes of up to DEAL_BATCH proofs (deal_pass_size) of
  // eight launches each, whatever the pass holds.  The five MsmMasks take three -- deal_msm_scalars_kernel, then
  // base_mul_few_kernel once over the G1 and once over the G2 share scalars -- and go to the caller's host buffers through
  // pinned staging while the five launches of the FFT and deg_red masks (deal_fr_masks_l) run on the same stream.
  static constexpr int DEAL_BATCH = DEGRED_BATCH;
  static constexpr size_t DEAL_WS_BYTES = (size_t)1 << 30;     // cap on the FFT masks' working memory per pass
  // proofs per pass: DEAL_BATCH (the batch limit of the king / deg_red kernels), fewer when 30 nb m elements of working
  // memory (the value vectors [l][6 nb][m/l] and the kings' output [n][6 nb][m/l]) would pass DEAL_WS_BYTES
  int deal_pass_size(int log_m) const {
    const size_t per_proof = (size_t)6 * (l + n) * (((size_t)1 << log_m) / l) * sizeof(Fr);
    return (int)std::max<size_t>(1, std::min<size_t>(DEAL_BATCH, DEAL_WS_BYTES / per_proof));
  }
  template <int L>
  int deal_fr_masks_l(int nb, int log_m, uint64_t seed, const zk_groth16_masks* mk, hipStream_t st) {
    const int log_lc = log_m - ilog2(l);
    const size_t Lc = (size_t)1 << log_lc;
    const uint32_t items = 6 * (uint32_t)nb;
    DealFftArg<Fr> fa{};
    DealDegredArg<Fr> da{};
    bool any_fft = false, any_dr = false;
    for (int b = 0; b < nb; b++) {
      for (int k = 0; k < 6; k++) {
        const int y = (k / 3) * 3 * nb + 3 * b + k % 3;
        fa.in_mask[y] = (Fr*)mk[b].fft_in[k];
        fa.out_mask[y] = (Fr*)mk[b].fft_out[k];
        any_fft = any_fft || fa.in_mask[y];
      }
      da.in_mask[b] = (Fr*)mk[b].degred_in;
      da.out_mask[b] = (Fr*)mk[b].degred_out;
      any_dr = any_dr || da.in_mask[b];
    }
    const unsigned kt = (unsigned)KING_THREADS;
    if (any_fft) {
      DevBuf& hwork_ = ws(st)->hwork;
      ZK_HIP(hwork_.ensure((size_t)items * (l + n) * Lc * sizeof(Fr)));
      Fr* vals = (Fr*)hwork_.p;                       // [l][items][Lc]
      Fr* kout = vals + (size_t)items * l * Lc;       // [n][items][Lc]
      deal_fft_fill_pack_kernel<FrP, L><<<dim3((unsigned)((Lc + kt - 1) / kt), items), dim3(kt), 0, st>>>(
          fa, (uint32_t)nb, (uint32_t)log_lc, rs(seed, 2ull * items), pmat_, pack2_, vals);
      ZK_HIP(hipGetLastError());
      const Fr w2m = root_of_unity(log_m + 1);
      for (int cfg = 0; cfg < 2; cfg++) {
        KingBatch<Fr> kb{};
        kb.stride = Lc;
        kb.row_pitch = (size_t)items * Lc;
        kb.items_per = 3;
        kb.seed_step = 16;
        kb.seed_xor = rng_replay_ ? 0x2222ull : 0ull;
        const size_t off = (size_t)cfg * 3 * nb * Lc;
        int rc = king_dispatch_batch(vals + off, kb, 3 * nb, l, log_m, cfg == 0, ident_, cfg == 0 ? &w2m : nullptr, 0,
                                     cfg == 0, seed + 3 * cfg, kout + off, true, st);
        if (rc) return rc;
      }
      deal_fft_scatter_kernel<Fr><<<dim3((unsigned)(((size_t)n * Lc + 255) / 256), items), dim3(256), 0, st>>>(kout, fa, items, Lc,
                                                                                                           (uint32_t)n);
      ZK_HIP(hipGetLastError());
    }
    if (any_dr) {
      deal_degred_kernel<FrP, L><<<dim3((unsigned)((Lc + kt - 1) / kt), (unsigned)nb), dim3(kt), 0, st>>>(
          da, Lc, rs(seed, 3ull * nb), pmat_, pack2_);
      ZK_HIP(hipGetLastError());
    }
    return ZK_OK;
  }
  int deal_masks_chunk(int nb, int log_m, const void* g1_gen, const void* g2_gen, uint64_t seed, const zk_groth16_masks* mk,
                       hipStream_t st) {
    using Fq = Fp<typename Cfg::FqP>;
    using Fq2 = Fp2<typename Cfg::FqP>;
    using J1 = Jacobian<Fq>;
    using J2 = Jacobian<Fq2>;
    bool any1 = false, any2 = false;
    for (int b = 0; b < nb; b++)
      for (int k = 0; k < 5; k++)
        if (mk[b].msm_in[k]) (k == 2 ? any2 : any1) = true;
    StreamWs* w_ = ws(st);
    const size_t per = (size_t)nb * 2 * n;                     // share scalars (= points) of one mask slot over the chunk
    const size_t sc_bytes = 5 * per * sizeof(Fr), p1_bytes = 4 * per * sizeof(J1), p2_bytes = per * sizeof(J2);
    if (any1 || any2) {
      ZK_HIP(w_->deal.ensure(sc_bytes + p1_bytes + p2_bytes));
      if (w_->deal_pin_bytes < p1_bytes + p2_bytes) {
        if (w_->deal_pin) (void)hipHostFree(w_->deal_pin);
        w_->deal_pin = nullptr, w_->deal_pin_bytes = 0;
        ZK_HIP(hipHostMalloc(&w_->deal_pin, p1_bytes + p2_bytes, hipHostMallocDefault));
        w_->deal_pin_bytes = p1_bytes + p2_bytes;
      }
      if (!w_->deal_ev) ZK_HIP(hipEventCreateWithFlags(&w_->deal_ev, hipEventDisableTiming));
      Fr* sc = (Fr*)w_->deal.p;
      char* pts = (char*)w_->deal.p + sc_bytes;
      const unsigned total = (unsigned)(5 * per);
      deal_msm_scalars_kernel<FrP><<<dim3((total + 63) / 64), dim3(64), 0, st>>>(rs(seed, 15ull * (uint64_t)nb), nb, l, t, n,
                                                                                pmat_, sc);
      ZK_HIP(hipGetLastError());
      if (any1) {
        int rc = base_mul_few_t<Fq>(g1_gen, sc, 4 * per, pts, st);
        if (rc) return rc;
        ZK_HIP(hipMemcpyAsync(w_->deal_pin, pts, p1_bytes, hipMemcpyDeviceToHost, st));
      }
      if constexpr (Cfg::HAS_G2) {
        if (any2) {
          int rc = base_mul_few_t<Fq2>(g2_gen, sc + 4 * per, per, pts + p1_bytes, st);
          if (rc) return rc;
          ZK_HIP(hipMemcpyAsync((char*)w_->deal_pin + p1_bytes, pts + p1_bytes, p2_bytes, hipMemcpyDeviceToHost, st));
        }
      }
      ZK_HIP(hipEventRecord(w_->deal_ev, st));
    }
    // the Fr masks of the chunk: one draw + pack launch for the 6 nb FFT value vectors and in-masks, one king launch per
    // configuration (k < 3: the d_ifft with the coset shift w_2m and rearranged output; k >= 3: the plain d_fft) over 3 nb
    // items, one launch that hands the kings' output to the callers' out-mask buffers, one launch for the DegRedMasks
    int rc = 0;
    switch (l) {
      case 1: rc = deal_fr_masks_l<1>(nb, log_m, seed, mk, st); break;
      case 2: rc = deal_fr_masks_l<2>(nb, log_m, seed, mk, st); break;
      case 4: rc = deal_fr_masks_l<4>(nb, log_m, seed, mk, st); break;
      default: rc = deal_fr_masks_l<8>(nb, log_m, seed, mk, st); break;
    }
    if (rc) return rc;
    if (any1 || any2) {
      ZK_HIP(hipEventSynchronize(w_->deal_ev));
      for (int kk = 0; kk < 5; kk++) {
        const int k = deal_msm_slot(kk);
        const size_t psz = k == 2 ? sizeof(J2) : sizeof(J1);
        const char* src = (const char*)w_->deal_pin + (k == 2 ? p1_bytes : (size_t)kk * per * sizeof(J1));
        for (int b = 0; b < nb; b++) {
          if (!mk[b].msm_in[k]) continue;
          memcpy((void*)mk[b].msm_in[k], src + (size_t)(2 * b) * n * psz, (size_t)n * psz);
          memcpy((void*)mk[b].msm_out[k], src + (size_t)(2 * b + 1) * n * psz, (size_t)n * psz);
        }
      }
    }
    return ZK_OK;
  }
  int groth16_deal_masks(int nproofs, int log_m, const void* g1_gen, const void* g2_gen, uint64_t seed,
                         const zk_groth16_masks* mk, hipStream_t st) override {
    if (nproofs < 1 || !mk) return fail(ZK_ERR_BAD_INPUT, "zk_groth16_deal_masks: nproofs < 1 or null masks");
    if (log_m < ilog2(l) || log_m + 1 > FrP::TWO_ADICITY) return fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT");
    for (int b = 0; b < nproofs; b++) {
      const zk_groth16_masks& m = mk[b];
      bool half = (m.degred_in != nullptr) != (m.degred_out != nullptr);
      for (int k = 0; k < 6; k++) half = half || (m.fft_in[k] != nullptr) != (m.fft_out[k] != nullptr);
      for (int k = 0; k < 5; k++) half = half || (m.msm_in[k] != nullptr) != (m.msm_out[k] != nullptr);
      if (half) return fail(ZK_ERR_BAD_INPUT, "zk_groth16_deal_masks: a mask slot needs both pointers or none");
      for (int k = 0; k < 5; k++) {
        if (!m.msm_in[k]) continue;
        if (k == 2 && (!Cfg::HAS_G2 || !g2_gen)) return fail(ZK_ERR_BAD_INPUT, "zk_groth16_deal_masks: no G2 generator for the G2 mask");
        if (k != 2 && !g1_gen) return fail(ZK_ERR_BAD_INPUT, "zk_groth16_deal_masks: no G1 generator");
      }
    }
    const int pass = deal_pass_size(log_m);
    for (int b0 = 0; b0 < nproofs; b0 += pass) {
      int rc = deal_masks_chunk(std::min(pass, nproofs - b0), log_m, g1_gen, g2_gen, seed + 16ull * (uint64_t)b0, mk + b0, st);
      if (rc) return rc;
    }
    return ZK_OK;
  }

  // ---------------------------------------------------------------- zk_groth16_deal_witness
  // QAP::pss (qap.rs:91-135) and the two pack_from_witness (sha256.rs:131-156) from a device-resident witness: r1cs_qap,
  // bit reversal and pack at order 1 with seeds + 0, 1, 2, then w[1:] (seed + 3) and w[ni:] (seed + 4) packed straight from
  // w_d with a zero tail.  With all five outputs NULL only the two chunk counts are returned.
  int groth16_deal_witness(const void* pa, const void* ca, const void* va, const void* pb, const void* cb, const void* vb,
                           const void* w, size_t nvars, size_t nc, size_t ni, int log_m, uint64_t seed, void* qa, void* qb,
                           void* qc, void* a_share, void* ax_share, size_t* len_a, size_t* len_w, hipStream_t st) override {
    if (nvars < 1 || ni < 1 || ni > nvars) return fail(ZK_ERR_BAD_INPUT, "bad R1CS dimensions");
    const size_t la = (nvars - 1 + l - 1) / l, lw = (nvars - ni + l - 1) / l;
    if (len_a) *len_a = la;
    if (len_w) *len_w = lw;
    if (!qa && !qb && !qc && !a_share && !ax_share) return ZK_OK;          // size query
    if (!qa || !qb || !qc || (la && !a_share) || (lw && !ax_share) || !w) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (log_m < ilog2(l) || log_m > 30) return fail(ZK_ERR_BAD_INPUT, "bad domain size");
    const size_t m = (size_t)1 << log_m;
    DevBuf& hwork_ = ws(st)->hwork;
    ZK_HIP(hwork_.ensure(3 * m * sizeof(Fr)));
    Fr* abc = (Fr*)hwork_.p;
    int rc = r1cs_qap(pa, ca, va, pb, cb, vb, w, nvars, nc, ni, log_m, abc, abc + m, abc + 2 * m, st);
    if (rc) return rc;
    void* const q[3] = {qa, qb, qc};
    for (int k = 0; k < 3; k++) {
      rc = bitrev(abc + k * m, log_m, st);
      if (!rc) rc = pss_pack(abc + k * m, m / l, 1, seed + k, false, q[k], st);
      if (rc) return rc;
    }
    rc = pss_pack_count((const Fr*)w + 1, nvars - 1, seed + 3, (Fr*)a_share, st);
    if (rc) return rc;
    return pss_pack_count((const Fr*)w + ni, nvars - ni, seed + 4, (Fr*)ax_share, st);
  }
