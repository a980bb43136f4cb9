// Part of class Engine<Cfg> (engine_impl.hpp includes this file INSIDE the class body): the issue callback of the per-party
// entry points (zk_party_*).  The rendezvous (party_rdv.hpp) hands the k records of one round, in ascending party order, to
// party_issue on the thread that arrived last; it turns them into the ONE rank call (dist_*) that exists:
//   1. the slot's own stream waits for the event every caller recorded on ITS stream when it arrived;
//   2. every operand whose k rows are the rows of one block (p[i] == p[0] + i * row_bytes) is passed as p[0] -- nothing is
//      copied, and a registered fixed-base table applies because the rank call sees the caller's own pointer; any other
//      operand is gathered into the slot's staging block by rows_gather_kernel (rows.hpp), one launch per group of equally
//      long rows (up to 96 rows each);
//   3. the rank call is issued on the slot's stream;
//   4. staged outputs are scattered back, the completion event is recorded, and every caller's stream waits for it.
// Nothing here takes a lock across the rank call: slots of different channels issue side by side (what they share in the
// engine is per channel or guarded around the mutation: DESIGN.md section 8, "shared state").

  struct PartyOperand {
    int idx;               // PartyRec::ptr index
    size_t row_bytes;
    bool in, out;          // read by the rank call / written by it
    void* resolved = nullptr;
    bool staged = false;
    size_t off = 0;        // byte offset of its [k][row] block in the staging buffer
  };

  PartyResult party_fail(int code, const std::string& m, int party = -1) {
    PartyResult r;
    r.code = fail(code, m, party);
    r.msg = m;
    r.party = party;
    return r;
  }

  // gather (scatter = false: operands the call reads) or scatter (operands it wrote) of the staged operands, grouped by row
  // length; ops are sorted by (row_bytes, offset), so the operands of one launch are one [items][k][row] block
  int party_rows(std::vector<PartyOperand*>& ops, const PartyRec* recs, int k, char* stage, bool scatter, hipStream_t s,
                 uint64_t* bytes) {
    const int per = ROWS_MAX / k;
    size_t i = 0;
    while (i < ops.size()) {
      RowTable t{};
      int items = 0;
      const size_t rb = ops[i]->row_bytes;
      char* block = stage + ops[i]->off;
      while (i < ops.size() && items < per && ops[i]->row_bytes == rb && stage + ops[i]->off == block + (size_t)items * k * rb) {
        for (int p = 0; p < k; p++) t.p[items * k + p] = (void*)recs[p].ptr[ops[i]->idx];
        items++;
        i++;
      }
      ZK_HIP(rows_launch(scatter, t, items * k, block, rb, s));
      *bytes += (uint64_t)items * k * rb;
    }
    return ZK_OK;
  }

  PartyResult party_issue(Net* net, PartyHub* hub, int sid, const PartyRec* recs) override {
    const int k = net->parties_per_rank();
    if (k != hub->k || k > PARTY_MAXK) return party_fail(ZK_ERR_BAD_INPUT, "party: the net drives more than 32 parties");
    PartyChan& ch = hub->chan[sid];
    Status cap;
    struct CaptureScope {
      explicit CaptureScope(Status* s) { IEngine::fail_capture = s; }
      ~CaptureScope() { IEngine::fail_capture = nullptr; }
    } scope(&cap);
    auto done = [&](int rc) {
      PartyResult r;
      r.code = rc;
      if (rc) {
        if (cap.code == ZK_OK) {                // raised on another thread (a pool task): the context's last message
          std::lock_guard<std::mutex> lk(last_mu);
          cap = last;
        }
        r.msg = cap.msg;
        r.party = cap.party;
      }
      return r;
    };
    auto hipdone = [&](hipError_t e, const char* where) { return done(hip_fail(e, where)); };
    if (!ch.stream) {
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
      hipError_t e = hipStreamCreateWithPriority(&ch.stream, hipStreamNonBlocking, hi);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ch.done, hipEventDisableTiming);
      if (e != hipSuccess) return hipdone(e, "party: stream / event");
    }
    const PartyRec& r0 = recs[0];
    const size_t fr = sizeof(Fr), fq = fq_bytes();
    const size_t aff = (r0.group == ZK_G2 ? 4 : 2) * fq, jac = (r0.group == ZK_G2 ? 6 : 3) * fq;
    // ---- the device operands of the call
    std::vector<PartyOperand> ops;
    auto add = [&](int idx, size_t row_bytes, bool in, bool out) { ops.push_back(PartyOperand{idx, row_bytes, in, out}); };
    size_t Lc = 0;
    switch (r0.op) {
      case PARTY_D_FFT:
      case PARTY_D_IFFT:
        if (r0.log2_m < ilog2(l) || r0.log2_m > FrP::TWO_ADICITY) return done(fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT"));
        Lc = ((size_t)1 << r0.log2_m) / l;
        add(0, Lc * fr, true, true), add(1, Lc * fr, true, false), add(2, Lc * fr, true, false);
        break;
      case PARTY_DEG_RED:
        add(0, r0.len * fr, true, true), add(1, r0.len * fr, true, false), add(2, r0.len * fr, true, false);
        break;
      case PARTY_D_PP:
        for (int i = 0; i < 4; i++) add(i, r0.len * fr, true, false);
        add(4, r0.len * fr, false, true);
        break;
      case PARTY_D_MSM:
        if (r0.group != ZK_G1 && r0.group != ZK_G2) return done(fail(ZK_ERR_BAD_INPUT, "bad group"));
        add(0, r0.len * aff, true, false), add(1, r0.len * fr, true, false);
        break;
      case PARTY_CIRCOM_H:
      case PARTY_PROVE: {
        if (r0.log2_m < ilog2(l) || r0.log2_m + 1 > FrP::TWO_ADICITY) return done(fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT"));
        Lc = ((size_t)1 << r0.log2_m) / l;
        for (int i = 0; i < 3; i++) add(i, Lc * fr, true, false);
        if (r0.op == PARTY_CIRCOM_H) {
          add(3, Lc * fr, false, true);
          for (int i = 4; i < 18; i++) add(i, Lc * fr, true, false);
        } else {
          // ext: len_a, len_w, len_u of the CRS share
          add(3, r0.ext[0] * fr, true, false), add(4, r0.ext[1] * fr, true, false);
          for (int i = 5; i < 19; i++) add(i, Lc * fr, true, false);
          add(19, r0.ext[0] * 2 * fq, true, false), add(20, r0.ext[0] * 2 * fq, true, false);
          add(21, r0.ext[0] * 4 * fq, true, false), add(22, r0.ext[1] * 2 * fq, true, false);
          add(23, r0.ext[2] * 2 * fq, true, false);
        }
        break;
      }
      default:
        return done(fail(ZK_ERR_BAD_INPUT, "party: unknown call"));
    }
    // ---- rows of one block, or staged
    size_t stage_bytes = 0;
    for (PartyOperand& o : ops) {
      if (!recs[0].ptr[o.idx] || !o.row_bytes) {      // NULL (the zero mask; NULL-ness agrees across the round) or empty
        o.resolved = (void*)recs[0].ptr[o.idx];
        continue;
      }
      bool rows_of_one_block = true;
      for (int p = 0; p < k; p++) {
        const char* q = (const char*)recs[p].ptr[o.idx];
        if ((uintptr_t)q & 15)
          return done(fail(ZK_ERR_BAD_INPUT, "party " + std::to_string(net->party(net->rank, p)) + ": a row is not 16-byte aligned",
                           net->party(net->rank, p)));
        if (q != (const char*)recs[0].ptr[o.idx] + (size_t)p * o.row_bytes) rows_of_one_block = false;
      }
      if (rows_of_one_block) o.resolved = (void*)recs[0].ptr[o.idx];
      else o.staged = true;
    }
    std::vector<PartyOperand*> gin, gout;
    {
      std::vector<PartyOperand*> st;
      for (PartyOperand& o : ops)
        if (o.staged) st.push_back(&o);
      std::stable_sort(st.begin(), st.end(), [](const PartyOperand* a, const PartyOperand* b) {
        if (a->row_bytes != b->row_bytes) return a->row_bytes < b->row_bytes;
        if (a->in != b->in) return a->in;                // inputs of one row length side by side, then its pure outputs
        return a->out < b->out;                          // ... and the in-place ones last among the inputs
      });
      for (PartyOperand* o : st) {
        if (o->row_bytes & 15) return done(fail(ZK_ERR_BAD_INPUT, "party: a staged row is not a multiple of 16 bytes"));
        o->off = stage_bytes;
        stage_bytes += (size_t)k * o->row_bytes;
        if (o->in) gin.push_back(o);
      }
      for (PartyOperand* o : st)
        if (o->out) gout.push_back(o);
    }
    if (stage_bytes) {
      hipError_t e = ch.stage.ensure(stage_bytes);
      if (e != hipSuccess) return hipdone(e, "party: staging buffer");
      for (PartyOperand& o : ops)
        if (o.staged) o.resolved = (char*)ch.stage.p + o.off;
    }
    // ---- 1. the slot's stream behind every caller's arrival
    for (int p = 0; p < k; p++) {
      hipError_t e = hipStreamWaitEvent(ch.stream, (hipEvent_t)recs[p].h[1], 0);
      if (e != hipSuccess) return hipdone(e, "party: wait for a caller's stream");
    }
    // ---- 2. stage in
    uint64_t moved = 0;
    int rc = party_rows(gin, recs, k, (char*)ch.stage.p, false, ch.stream, &moved);
    if (rc) return done(rc);
    // ---- 3. the rank call
    auto R = [&](int idx) -> void* {
      for (PartyOperand& o : ops)
        if (o.idx == idx) return o.resolved;
      return nullptr;
    };
    // host rows (MSM masks and outputs: one Jacobian point per party) as one vector per operand
    auto host_in = [&](int idx, size_t bytes, std::vector<char>& buf) -> const void* {
      if (!recs[0].ptr[idx]) return nullptr;
      buf.resize((size_t)k * bytes);
      for (int p = 0; p < k; p++) memcpy(buf.data() + (size_t)p * bytes, recs[p].ptr[idx], bytes);
      return buf.data();
    };
    auto host_out = [&](int idx, size_t bytes, const std::vector<char>& buf) {
      for (int p = 0; p < k; p++) memcpy((void*)recs[p].ptr[idx], buf.data() + (size_t)p * bytes, bytes);
    };
    hipStream_t s = ch.stream;
    switch (r0.op) {
      case PARTY_D_FFT:
      case PARTY_D_IFFT:
        rc = dist_d_fft(net, sid, R(0), R(1), R(2), r0.rearrange, r0.log2_m, r0.op == PARTY_D_IFFT ? 1 : 0,
                        r0.g_len ? (const void*)r0.g : nullptr, r0.seed, s);
        break;
      case PARTY_DEG_RED:
        rc = dist_deg_red(net, sid, R(0), R(1), R(2), r0.len, r0.seed, s);
        break;
      case PARTY_D_PP:
        rc = dist_d_pp(net, sid, R(0), R(1), R(2), R(3), r0.len, r0.seed, R(4), s);
        break;
      case PARTY_D_MSM: {
        std::vector<char> mi, mo, out((size_t)k * jac);
        for (int p = 0; p < k; p++)
          if (!recs[p].ptr[4]) return done(fail(ZK_ERR_BAD_INPUT, "null output"));
        rc = dist_d_msm(net, sid, r0.group, R(0), R(1), r0.len, host_in(2, jac, mi), host_in(3, jac, mo), out.data(), s);
        if (!rc) host_out(4, jac, out);
        break;
      }
      case PARTY_CIRCOM_H: {
        zk_groth16_masks mk{};
        for (int i = 0; i < 6; i++) mk.fft_in[i] = R(4 + i), mk.fft_out[i] = R(10 + i);
        mk.degred_in = R(16), mk.degred_out = R(17);
        rc = dist_circom_h(net, R(0), R(1), R(2), r0.log2_m, &mk, r0.seed, R(3), s);
        break;
      }
      case PARTY_PROVE: {
        zk_groth16_masks mk{};
        for (int i = 0; i < 6; i++) mk.fft_in[i] = R(5 + i), mk.fft_out[i] = R(11 + i);
        mk.degred_in = R(17), mk.degred_out = R(18);
        const size_t j1 = 3 * fq, j2 = 6 * fq;
        std::vector<char> hin[5], hout[5], pa((size_t)k * j1), pb((size_t)k * j2), pc((size_t)k * j1);
        for (int i = 0; i < 5; i++) {
          mk.msm_in[i] = host_in(24 + i, i == 2 ? j2 : j1, hin[i]);
          mk.msm_out[i] = host_in(29 + i, i == 2 ? j2 : j1, hout[i]);
        }
        // the single CRS elements (a_query0, delta_g1, ...) are taken from the rank's first party
        zk_crs_share crs = *(const zk_crs_share*)recs[0].caller;
        crs.s_d = R(19), crs.h_d = R(20), crs.v_d = R(21), crs.w_d = R(22), crs.u_d = R(23);
        for (int p = 0; p < k; p++)
          if (!recs[p].ptr[34] || !recs[p].ptr[35] || !recs[p].ptr[36]) return done(fail(ZK_ERR_BAD_INPUT, "null pointer"));
        rc = dist_prove(net, &crs, R(0), R(1), R(2), R(3), R(4), r0.g, r0.g + fr, r0.log2_m, &mk, r0.seed, pa.data(), pb.data(),
                        pc.data(), s);
        if (!rc) host_out(34, j1, pa), host_out(35, j2, pb), host_out(36, j1, pc);
        break;
      }
    }
    rc = dist_finish(net, rc);
    if (rc) return done(rc);
    // ---- 4. stage out, completion, and every caller's stream behind it
    rc = party_rows(gout, recs, k, (char*)ch.stage.p, true, ch.stream, &moved);
    if (rc) return done(rc);
    hipError_t e = hipEventRecord(ch.done, ch.stream);
    // (a slot that failed meanwhile: its waiters gave up on this call and are gone -- their streams are not touched)
    const bool gone = hub->slot[sid].failed();
    for (int p = 0; p < k && e == hipSuccess && !gone; p++) e = hipStreamWaitEvent((hipStream_t)recs[p].h[0], ch.done, 0);
    if (e != hipSuccess) return hipdone(e, "party: completion event");
    hub->stats[0]++;
    hub->stats[stage_bytes ? 2 : 1]++;
    hub->stats[3] += moved;
    return done(ZK_OK);
  }
