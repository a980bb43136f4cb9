// Part of class Engine<Cfg> (engine_impl.hpp includes this file INSIDE the class body): the local h chain -- circom_h in
// every form, described by an HChain and run by the one driver h_chain -- and libsnark_h.  Not a stand-alone header.

  // ---------------------------------------------------------------- circom_h (ext_wit.rs:104-181)
  // Three d_ifft (rearranged, g = w_2m), three d_fft, h = a*b - c share-wise, deg_red -- for nb proofs as ONE launch chain:
  // the 3 nb vectors go through every NTT pass, king and deg_red launch together (grid.y).  Proof b draws the randomness a
  // single proof with seed + PROOF_SEED_STEP * b draws.
  //
  // The checked chain (a report) repairs each of a proof's seven king words before the king reads it.  Items 0..2: the d_ifft
  // words of a, b, c; 3..5: the d_fft words; 6: the deg_red word.  The words are those of the single-word checked calls
  // (engine_gao.inc.hpp d_fft_checked, deg_red_checked): fft1(x) / m + in_mask (without a mask fft1(x), the 1 / m in the
  // king's table), fft1(x) + in_mask, a*b - c + in_mask.  Each is materialised in the work buffer, so the kings run with null
  // in-masks; a round's 3 nb words are repaired by ONE gao_run (a full batch is exactly GAO_BATCH_MAX items) at dimension
  // 2l, the nb deg_red words by one at 4l - 1: detection only.  The unchecked chain has no word step and no repair: the
  // in-masks go to the king and the product is formed at deg_red's load.
  struct HReport {
    uint8_t* status;        // [nb][7][m/l], proof-major
    uint32_t* errpos;       // [nb][7][m/l] or null
    uint64_t* summary;      // [nb][7][3 + n] or null
    const uint32_t* ids = nullptr;      // zk_*_checked_parties: the party list (checked_list has passed it), np < n of them;
    int np = 0;                         // 0: all n parties
  };
  static constexpr uint32_t PROOF_SEED_STEP = 16;
  static_assert(H_BATCH_MAX == DEGRED_BATCH && H_BATCH_ITEMS == KING_BATCH && H_BATCH_ITEMS == GAO_BATCH_MAX,
                "one round of a full batch is one king launch and one repair call");
  static_assert(sizeof(Fr) % 32 == 0, "the repair's working memory stays aligned behind the vectors");
  static HReport report_slice(const HReport& rep, int b, size_t Lc, int n_) {
    return HReport{rep.status + (size_t)b * H_REPORT_ROWS * Lc, rep.errpos ? rep.errpos + (size_t)b * H_REPORT_ROWS * Lc : nullptr,
                   rep.summary ? rep.summary + (size_t)b * H_REPORT_ROWS * (3 + n_) : nullptr};
  }
  struct HChain {
    int nb;                                  // proofs, 1 .. H_BATCH_MAX
    const void* const* qa;                   // [nb] device vectors [n][m/l]; a single proof is an array of one
    const void* const* qb;
    const void* const* qc;
    int log_m;
    const zk_groth16_masks* mk;              // nb mask sets or null
    uint64_t seed;
    Fr* h;                                   // [nb][n][m/l]
    const HReport* rep;                      // null: the unchecked chain.  With a party list (np < n): nb == 1
    DevBuf* hwork;
    hipStream_t st;
  };
  bool h_listed(const HChain& c) const { return c.rep && c.rep->np > 0 && c.rep->np < n; }
  // every refusal of a chain, before anything is written
  int h_refuse(const HChain& c) {
    if (c.nb < 1 || c.nb > H_BATCH_MAX) return fail(ZK_ERR_BAD_INPUT, "batch size must be in 1.." + std::to_string(H_BATCH_MAX));
    if (c.log_m < ilog2(l)) return fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT");
    if (c.log_m + 1 > FrP::TWO_ADICITY) return fail(ZK_ERR_BAD_INPUT, "domain too large for this field");
    bool null = !c.qa || !c.qb || !c.qc || !c.h || (c.rep && !c.rep->status);
    for (int b = 0; b < c.nb && !null; b++) null = !c.qa[b] || !c.qb[b] || !c.qc[b];
    if (null) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (c.rep && !gao_batch_fits(3 * (uint64_t)c.nb, ((size_t)1 << c.log_m) / l))
      return fail(ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks in the batch");
    if (h_listed(c) && c.nb > 1) return fail(ZK_ERR_BAD_INPUT, "a party list takes one proof");
    return ZK_OK;
  }
  // one launch per step needs the in-masks of a round present or absent alike across the batch and the round's three words
  static bool h_uniform(int nb, const zk_groth16_masks* mk) {
    for (int k = 0; mk && k < 6; k++)
      for (int b = 0; b < nb; b++)
        if ((mk[b].fft_in[k] != nullptr) != (mk[0].fft_in[k - k % 3] != nullptr)) return false;
    return true;
  }
  // The king of a round over `items` words at in + y * per -> out + y * per, item y = 3 b + k with the randomness seed +
  // PROOF_SEED_STEP * b + k.  in_masks: the in-masks go to the king (the unchecked chain); null: they are in the words, and
  // so is the 1 / m of a masked word of the inverse round.  One batched launch when the in-masks and the 1 / m sit alike in
  // all words, a launch per word otherwise.
  int h_king(const Fr* in, int items, int np, const Fr* U, const Fr* const* in_masks, const Fr* const* out_masks,
             const bool* masked, int log_m, int inverse, const void* g, uint64_t seed, Fr* out, size_t per, hipStream_t st) {
    KingBatch<Fr> kb{};
    kb.stride = per;
    kb.items_per = 3;
    kb.seed_step = PROOF_SEED_STEP;
    bool alike = true;
    for (int y = 0; y < items; y++) {
      kb.in_mask[y] = in_masks ? in_masks[y] : nullptr;
      kb.out_mask[y] = out_masks[y];
      alike = alike && masked[y] == masked[0];
    }
    auto scale = [&](int y) { return inverse && (in_masks || !masked[y]) ? 1 : 0; };
    if (alike || (!in_masks && !inverse))
      return king_dispatch_batch(in, kb, items, np, log_m, inverse, U, g, scale(0), inverse, seed, out, false, st);
    for (int y = 0; y < items; y++) {
      int rc = king_dispatch(in + y * per, kb.in_mask[y], np, log_m, inverse, U, g, scale(y), inverse, seed + kb.seed_off(y),
                             out + y * per, kb.out_mask[y], false, st);
      if (rc) return rc;
    }
    return ZK_OK;
  }

  // ---- the hooks of the chain with a party list (zk_circom_h_checked_parties, np == n - 1, one proof): only the words of
  // the listed parties reach the kings.  A round's three words are COMPACT, [np][m/l] at W0 + k * per, transformed out of
  // place (round 1 from the caller's vectors, round 2 from W1), and both kings write W1.  The batched king reads np rows at
  // the row pitch m/l from in + k * stride and writes n rows at out + k * stride, so the compact layout at the stride of the
  // full one goes through ONE batched launch.
  // The transform: at l <= 4 a round's 3 np row pointers go into one NttSrc as 3 n - 1 <= 47 vectors: vector k n + r is
  // listed row r of word k, and the one row of an item beyond its np -- never read by the repair or the king -- transforms
  // listed row 0 once more, so the three words of a round stay one set of NTT launches.  At l = 8 (93 pointers) one word per
  // call.
  int h_list_words(Fr* W, const Fr* const* src, int log_m, int inverse, size_t per, const uint32_t* ids, int np,
                   hipStream_t st) {
    const size_t Lc = ((size_t)1 << log_m) / l;
    int rc;
    if (3 * n - 1 <= NTT_SRC_MAX) {
      NttSrc<Fr> s{};
      s.per = 1;
      for (int k = 0; k < 3; k++)
        for (int r = 0; r < n && k * n + r < 3 * n - 1; r++) s.p[k * n + r] = src[k] + (size_t)ids[r < np ? r : 0] * Lc;
      return fft1_src(W, log_m, inverse, (size_t)(3 * n - 1), nullptr, st, s);
    }
    static_assert(GAO_MAX_N <= NTT_SRC_MAX, "one pointer per listed row");
    for (int k = 0; k < 3; k++) {
      NttSrc<Fr> s{};
      s.per = 1;
      for (int r = 0; r < np; r++) s.p[r] = src[k] + (size_t)ids[r] * Lc;
      if ((rc = fft1_src(W + k * per, log_m, inverse, (size_t)np, nullptr, st, s))) return rc;
    }
    return ZK_OK;
  }
  // The product: a*b - c + in_mask over the listed rows of W1, compact into W0: the one absent party e splits the rows into
  // those below it and those above, which move up by one.  Item 6: with n - 1 parties the dimension 4l - 1 leaves no
  // redundancy -- NOT CHECKED: the compact word goes to deg_red with the list unrepaired, its status and errpos bytes are 0
  // and its summary row is all zeros (no chunk checked; a clean item reads [m/l, 0, 0, ..]).
  int h_list_product(Fr* W0, const Fr* W1, const Fr* in_mask, const HReport& rep, size_t Lc, hipStream_t st) {
    const size_t per = (size_t)n * Lc;
    const uint32_t* ids = rep.ids;
    const int np = rep.np;
    uint32_t e = 0;
    while (e < (uint32_t)np && ids[e] == e) e++;
    int rc = vec_mul_sub(W0, W1, W1 + per, W1 + 2 * per, e * Lc, st);
    if (rc) return rc;
    const size_t up = (size_t)(e + 1) * Lc;
    if ((rc = vec_mul_sub(W0 + e * Lc, W1 + up, W1 + per + up, W1 + 2 * per + up, ((size_t)np - e) * Lc, st))) return rc;
    if ((rc = add_list_rows(W0, per, &in_mask, 1, ids, np, false, Fr::one(), Lc, st))) return rc;
    ZK_HIP(hipMemsetAsync(rep.status + 6 * Lc, 0, Lc, st));
    if (rep.errpos) ZK_HIP(hipMemsetAsync(rep.errpos + 6 * Lc, 0, Lc * 4, st));
    if (rep.summary) ZK_HIP(hipMemsetAsync(rep.summary + (size_t)6 * (3 + n), 0, (size_t)(3 + n) * 8, st));
    return ZK_OK;
  }

  // The driver.  A round is transform -> (checked: words -> repair) -> king; the inverse round, the forward round, then the
  // product and deg_red.  The forms differ in the three hooks only -- transform, words, product:
  //   unchecked      in place in W0 / W1 (the first pass reads the caller's vectors, no copy); no words; the product at
  //                  deg_red's load (mul_b / sub_c)
  //   checked        the same transforms; ONE h_words_batch_kernel launch per round with a mask (it scales and adds where
  //                  there is one, so partial mask sets need nothing else); ONE h_mulsub_batch_kernel launch into W1, which
  //                  the second king has read
  //   party list     h_list_words, add_list_rows, h_list_product
  // Refusals, the layout of hwork (h_batch.hpp h_layout), the repair, the king and deg_red are shared.
  // The repair indexes status and errpos by item, so a round's rows are contiguous while the caller's report is proof-major:
  // a batch writes a round-major staging report behind the repair's working memory (staging_row) and
  // h_report_gather_kernel, its last launch, moves the rows to the caller's buffers.  One proof needs neither:
  // staging_row(1, 0, k) == k, so its repairs write the caller's report.
  // A batch whose in-masks are not uniform (h_uniform) runs proof by proof on the stream -- the same results.
  int h_chain(const HChain& c) {
    int rc = h_refuse(c);
    if (rc) return rc;
    const int nb = c.nb, log_m = c.log_m, items = 3 * nb;
    const size_t Lc = ((size_t)1 << log_m) / l, per = (size_t)n * Lc;
    const zk_groth16_masks* mk = c.mk;
    hipStream_t st = c.st;
    if (nb > 1 && !h_uniform(nb, mk)) {
      for (int b = 0; b < nb; b++) {
        HChain one = c;
        HReport rb{};
        one.nb = 1, one.qa += b, one.qb += b, one.qc += b, one.mk += b, one.h += b * per;
        one.seed += (uint64_t)PROOF_SEED_STEP * b;
        if (c.rep) rb = report_slice(*c.rep, b, Lc, n), one.rep = &rb;
        if ((rc = h_chain(one))) return rc;
      }
      return ZK_OK;
    }
    const bool checked = c.rep != nullptr, listed = h_listed(c);
    const uint32_t* ids = listed ? c.rep->ids : nullptr;
    const int np = listed ? c.rep->np : n;
    const Fr* U = nullptr;
    if ((rc = umat_for(ids, np, &U))) return rc;
    const HLayout lay = h_layout(n, nb, Lc, sizeof(Fr), checked ? gao_layout<Fr>(n, items, Lc, listed).bytes : 0,
                                 checked && c.rep->errpos, checked && c.rep->summary);
    ZK_HIP(c.hwork->ensure(lay.bytes));
    char* base = (char*)c.hwork->p;
    Fr* W0 = (Fr*)base;
    Fr* W1 = (Fr*)(base + lay.w1);
    // the report the repairs write: the caller's, or the staging rows of a batch
    HReport out = checked ? *c.rep : HReport{};
    if (checked && nb > 1)
      out = HReport{(uint8_t*)(base + lay.status), out.errpos ? (uint32_t*)(base + lay.errpos) : nullptr,
                    out.summary ? (uint64_t*)(base + lay.summary) : nullptr};
    auto repair = [&](Fr* W, int round, int dimension) {
      const size_t first = staging_round_first((uint32_t)nb, (uint32_t)round);
      GaoCall g = gao_call(W, ids, np, Lc, dimension, out.status + first * Lc, out.errpos ? out.errpos + first * Lc : nullptr,
                           out.summary ? out.summary + first * (3 + n) : nullptr);
      g.nitems = (int)staging_round_items((uint32_t)nb, (uint32_t)round), g.item_stride = per;
      return gao_run<FrP, true>(this, base + lay.gao, l, g, st);
    };
    const Fr w2m = root_of_unity(log_m + 1);     // Radix2EvaluationDomain::new(2m).element(1), ext_wit.rs:120-125
    const Fr minv = checked ? Fr::from_u64((uint64_t)1 << log_m).inverse() : Fr::one();
    // round 0: 3 nb x d_ifft(rearrange = true, g = w_2m) (ext_wit.rs:127-159); round 1: 3 nb x d_fft(rearrange = false)
    // (ext_wit.rs:161-170)
    for (int round = 0; round < 2; round++) {
      const int inverse = !round, first = 3 * round;
      Fr* W = listed || !round ? W0 : W1;
      Fr* next = W == W0 ? W1 : W0;
      const Fr* in_mask[H_BATCH_ITEMS];
      const Fr* out_mask[H_BATCH_ITEMS];
      bool masked[H_BATCH_ITEMS], any = false;
      for (int y = 0; y < items; y++) {
        in_mask[y] = mk ? (const Fr*)mk[y / 3].fft_in[first + y % 3] : nullptr;
        out_mask[y] = mk ? (const Fr*)mk[y / 3].fft_out[first + y % 3] : nullptr;
        any = (masked[y] = in_mask[y] != nullptr) || any;
      }
      // transform
      if (listed) {
        const Fr* q[3] = {(const Fr*)c.qa[0], (const Fr*)c.qb[0], (const Fr*)c.qc[0]};
        const Fr* w[3] = {W1, W1 + per, W1 + 2 * per};
        rc = h_list_words(W, round ? w : q, log_m, inverse, per, ids, np, st);
      } else if (!round) {
        NttSrc<Fr> src{};
        src.per = (uint32_t)n;
        for (int b = 0; b < nb; b++)
          src.p[3 * b] = (const Fr*)c.qa[b], src.p[3 * b + 1] = (const Fr*)c.qb[b], src.p[3 * b + 2] = (const Fr*)c.qc[b];
        rc = fft1_src(W, log_m, 1, (size_t)n * items, nullptr, st, src);
      } else {
        rc = fft1(W, log_m, 0, (size_t)n * items, nullptr, st);
      }
      if (rc) return rc;
      // words, repair
      if (listed) {
        if ((rc = add_list_rows(W, per, in_mask, 3, ids, np, inverse != 0, minv, Lc, st))) return rc;
      } else if (checked && any) {
        HWordMasks<Fr> hm{};
        for (int y = 0; y < items; y++) hm.mask[y] = in_mask[y];
        h_words_batch_kernel<Fr><<<h_batch_grid(per, items), dim3(256), 0, st>>>(W, per, hm, inverse, minv, per);
        ZK_HIP(hipGetLastError());
      }
      if (checked && (rc = repair(W, round, 2 * l))) return rc;
      // king
      if ((rc = h_king(W, items, np, U, checked ? nullptr : in_mask, out_mask, masked, log_m, inverse, inverse ? &w2m : nullptr,
                       c.seed + first, next, per, st)))
        return rc;
    }
    // h = a*b - c share-wise, then deg_red (ext_wit.rs:173-179)
    DegredBatch<Fr> db{};
    for (int b = 0; b < nb; b++) db.out_mask[b] = mk ? (const Fr*)mk[b].degred_out : nullptr;
    db.in_step = checked ? per : 3 * per;
    db.out_step = per;
    db.seed_step = PROOF_SEED_STEP;
    if (!checked) {
      for (int b = 0; b < nb; b++) db.in_mask[b] = mk ? (const Fr*)mk[b].degred_in : nullptr;
      return deg_red_batch(W0, db, nb, nullptr, n, Lc, c.seed + 6, c.h, st, 0, 0, W0 + per, W0 + 2 * per);
    }
    Fr* word = listed ? W0 : W1;
    if (listed) {
      if ((rc = h_list_product(W0, W1, mk ? (const Fr*)mk->degred_in : nullptr, *c.rep, Lc, st))) return rc;
    } else {
      HProdMasks<Fr> pm{};
      for (int b = 0; b < nb; b++) pm.mask[b] = mk ? (const Fr*)mk[b].degred_in : nullptr;
      h_mulsub_batch_kernel<Fr><<<h_batch_grid(per, nb), dim3(256), 0, st>>>(W1, per, W0, 3 * per, pm, per);
      ZK_HIP(hipGetLastError());
      if ((rc = repair(W1, 2, 4 * l - 1))) return rc;
    }
    if ((rc = deg_red_batch(word, db, nb, ids, np, Lc, c.seed + 6, c.h, st))) return rc;
    if (nb > 1) {
      h_report_gather_kernel<<<h_batch_grid(Lc, H_REPORT_ROWS * nb), dim3(256), 0, st>>>(
          (uint32_t)nb, (uint32_t)Lc, (uint32_t)(3 + n), out.status, out.errpos, out.summary, c.rep->status, c.rep->errpos,
          c.rep->summary);
      ZK_HIP(hipGetLastError());
    }
    return ZK_OK;
  }

  // ---- the entry points: each fills the descriptor
  int circom_h(const void* qa, const void* qb, const void* qc, int log_m, const zk_groth16_masks* mk, uint64_t seed,
               void* h, hipStream_t st) override {
    return h_chain(HChain{1, &qa, &qb, &qc, log_m, mk, seed, (Fr*)h, nullptr, &ws(st)->hwork, st});
  }
  int circom_h_checked(const void* qa, const void* qb, const void* qc, int log_m, const zk_groth16_masks* mk, uint64_t seed,
                       void* h, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    const HReport rep{status, errpos, summary};
    return h_chain(HChain{1, &qa, &qb, &qc, log_m, mk, seed, (Fr*)h, &rep, &ws(st)->hwork, st});
  }
  // all n parties (the chain above) or n - 1 of them (checked_list)
  int circom_h_checked_parties(const uint32_t* parties, int np, const void* qa, const void* qb, const void* qc, int log_m,
                               const zk_groth16_masks* mk, uint64_t seed, void* h, uint8_t* status, uint32_t* errpos,
                               uint64_t* summary, hipStream_t st) override {
    uint32_t ids[GAO_MAX_N];
    int rc = checked_list(parties, np, 2 * l, ids);
    if (rc) return rc;
    HReport rep{status, errpos, summary};
    if (np < n) rep.ids = ids, rep.np = np;
    return h_chain(HChain{1, &qa, &qb, &qc, log_m, mk, seed, (Fr*)h, &rep, &ws(st)->hwork, st});
  }
  int circom_h_batch_checked(int nb, const void* const* qa, const void* const* qb, const void* const* qc, int log_m,
                             const zk_groth16_masks* mk, uint64_t seed, void* h, uint8_t* status, uint32_t* errpos,
                             uint64_t* summary, hipStream_t st) override {
    const HReport rep{status, errpos, summary};
    return h_chain(HChain{nb, qa, qb, qc, log_m, mk, seed, (Fr*)h, &rep, &ws(st)->hwork, st});
  }

  // ---------------------------------------------------------------- libsnark_h (ext_wit.rs:14-102)
  // 3 x d_ifft with the coset shift g = F::GENERATOR (rearranged) -> 3 x d_fft (rearranged) -> (a*b - c) / Z(g) ->
  // d_ifft with g^-1.  Seven masks (or NULL arrays for FftMask::zero).
  int libsnark_h(const void* qa, const void* qb, const void* qc, int log_m, const void* const* fft_in,
                 const void* const* fft_out, uint64_t seed, void* h, hipStream_t st) override {
    if (log_m < ilog2(l) || log_m > FrP::TWO_ADICITY) return fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT");
    if (!qa || !qb || !qc || !h) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    const size_t Lc = ((size_t)1 << log_m) / l, per = (size_t)n * Lc;
    DevBuf& hwork_ = ws(st)->hwork;
    ZK_HIP(hwork_.ensure(6 * per * sizeof(Fr)));
    Fr* W0 = (Fr*)hwork_.p;
    Fr* W1 = W0 + 3 * per;
    const void* q[3] = {qa, qb, qc};
    for (int k = 0; k < 3; k++) ZK_HIP(hipMemcpyAsync(W0 + k * per, q[k], per * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    Fr g = generator();
    auto mi = [&](int k) { return fft_in ? fft_in[k] : nullptr; };
    auto mo = [&](int k) { return fft_out ? fft_out[k] : nullptr; };
    int rc;
    for (int k = 0; k < 3; k++) {
      rc = d_fft(W0 + k * per, mi(k), mo(k), 1, log_m, 1, &g, seed + k, W1 + k * per, st);
      if (rc) return rc;
      rc = d_fft(W1 + k * per, mi(3 + k), mo(3 + k), 1, log_m, 0, nullptr, seed + 3 + k, W0 + k * per, st);
      if (rc) return rc;
    }
    rc = vec_mul_sub(W1, W0, W0 + per, W0 + 2 * per, per, st);
    if (rc) return rc;
    // 1 / Z(g), Z(x) = x^m - 1  (ext_wit.rs:78-81)
    Fr zinv = (g.pow_u64((uint64_t)1 << log_m) - Fr::one()).inverse();
    rc = vec_scale(W1, &zinv, per, st);
    if (rc) return rc;
    Fr ginv = g.inverse();
    return d_fft(W1, mi(6), mo(6), 0, log_m, 1, &ginv, seed + 6, h, st);
  }

