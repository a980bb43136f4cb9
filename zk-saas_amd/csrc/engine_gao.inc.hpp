// Part of class Engine<Cfg> (engine_impl.hpp includes this file INSIDE the class body): zk_pss_unpack_robust and
// zk_pss_unpack_robust_parties, the error-correcting unpack; zk_pss_repair, zk_pss_repair_parties and the checked king rounds built on them.  Kernels and driver: gao_impl.hpp, compiled in gao_<curve>.hip.  Not a stand-alone header.

  // ---------------------------------------------------------------- zk_pss_unpack_robust
  // shares [n][nchunks] of all n parties; any of secrets, message, errpos, summary may be null.  Working memory is the caller
  // stream's hwork (StreamWs); no host synchronisation.
  int pss_unpack_robust(const void* shares, size_t nchunks, int dimension, void* secrets, void* message, uint8_t* status,
                        uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    return gao_unpack_robust_run<FrP>(this, ws(st)->hwork, l, shares, nchunks, dimension, secrets, message, status, errpos,
                                      summary, st);
  }

  // ---------------------------------------------------------------- zk_pss_unpack_robust_parties
  // shares [nparties][nchunks] of the listed parties (ascending ids; null: 0 .. nparties - 1); the rest as above
  int pss_unpack_robust_parties(const void* shares, const uint32_t* parties, int nparties, size_t nchunks, int dimension,
                                void* secrets, void* message, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                                hipStream_t st) override {
    return gao_unpack_robust_parties_run<FrP>(this, ws(st)->hwork, l, shares, parties, nparties, nchunks, dimension, secrets,
                                              message, status, errpos, summary, st);
  }

  // ---------------------------------------------------------------- zk_pss_repair
  // shares [n][nchunks] of all n parties, in place: status, errpos and summary are pss_unpack_robust's; in a corrected chunk the
  // share of every party named in errpos becomes h(w_n^p), every other element keeps its bytes.  Same working memory, no host
  // synchronisation.
  int pss_repair(void* shares, size_t nchunks, int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                 hipStream_t st) override {
    return gao_repair_run<FrP>(this, ws(st)->hwork, l, shares, nchunks, dimension, status, errpos, summary, st);
  }

  // ---------------------------------------------------------------- zk_pss_repair_batch
  // nitems matrices [n][nchunks], item i at shares + i * item_stride (KingBatch::stride; circom_h's W0 / W1): pss_repair of
  // each, with ONE clear, ONE scan launch (the item on grid.y) and ONE decoder launch over one list of dirty (item, chunk)
  // entries.  status / errpos [nitems][nchunks], summary [nitems][3 + n].  A refusal writes nothing.
  static_assert(GAO_BATCH_MAX == KING_BATCH, "a repair batch takes the items of a king batch");
  int repair_batch_check(const void* shares, size_t item_stride, int nitems, size_t nchunks, int dimension,
                         const uint8_t* status) {
    if (nitems < 1 || nitems > KING_BATCH) return fail(ZK_ERR_BAD_INPUT, "bad repair batch");
    if (dimension < 1 || dimension > n - 1) return fail(ZK_ERR_BAD_INPUT, "dimension must lie in 1 .. n - 1");
    if (nchunks == 0) return ZK_OK;
    if (!shares || !status) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (!gao_batch_fits((uint64_t)nitems, nchunks)) return fail(ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks in the batch");
    if (item_stride < (size_t)n * nchunks) return fail(ZK_ERR_BAD_INPUT, "item stride below n * nchunks");
    return ZK_OK;
  }
  int pss_repair_batch(void* shares, size_t item_stride, int nitems, size_t nchunks, int dimension, uint8_t* status,
                       uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    int rc = repair_batch_check(shares, item_stride, nitems, nchunks, dimension, status);
    if (rc || !nchunks) return rc;
    DevBuf& wk = ws(st)->hwork;
    ZK_HIP(wk.ensure(gao_batch_work_bytes(n, nitems, nchunks)));
    return gao_repair_batch_run<FrP>(this, wk.p, l, shares, item_stride, nitems, nchunks, dimension, status, errpos, summary,
                                     st);
  }

  // ---------------------------------------------------------------- zk_pss_repair_batch_parties
  // nitems compact matrices [nparties][nchunks] of ONE party list, item i at shares + i * item_stride: pss_repair_parties of
  // each with the launches of pss_repair_batch and the two tables of the list, put into working memory once per call.  The
  // refusals are pss_repair_parties' (list, dimension, too few shares) and pss_repair_batch's; a refusal writes nothing.
  int repair_list_check(const uint32_t* parties, int np, int dimension, uint32_t* ids) {
    if (np <= 0 || np > n) return fail(ZK_ERR_BAD_INPUT, "bad party count");
    for (int i = 0; i < np; i++) {
      ids[i] = parties ? parties[i] : (uint32_t)i;
      if (ids[i] >= (uint32_t)n || (i > 0 && ids[i] <= ids[i - 1]))
        return fail(ZK_ERR_BAD_INPUT, "party ids must be ascending and < n");
    }
    if (dimension < 1 || dimension > n - 1) return fail(ZK_ERR_BAD_INPUT, "dimension must lie in 1 .. n - 1");
    if (np <= dimension) return fail(ZK_ERR_PROTOCOL, "Not enough shares to reconstruct");      // pss.rs:183-186
    return ZK_OK;
  }
  int pss_repair_batch_parties(void* shares, const uint32_t* parties, int np, size_t item_stride, int nitems, size_t nchunks,
                               int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    uint32_t ids[GAO_MAX_N];
    int rc = repair_list_check(parties, np, dimension, ids);
    if (rc) return rc;
    if (np == n) return pss_repair_batch(shares, item_stride, nitems, nchunks, dimension, status, errpos, summary, st);
    if (nitems < 1 || nitems > KING_BATCH) return fail(ZK_ERR_BAD_INPUT, "bad repair batch");
    if (nchunks == 0) return ZK_OK;
    if (!shares || !status) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (!gao_batch_fits((uint64_t)nitems, nchunks)) return fail(ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks in the batch");
    if (item_stride < (size_t)np * nchunks) return fail(ZK_ERR_BAD_INPUT, "item stride below nparties * nchunks");
    DevBuf& wk = ws(st)->hwork;
    ZK_HIP(wk.ensure(gao_batch_parties_work<Fr>(n, nitems, nchunks).bytes));
    return gao_repair_batch_parties_run<FrP>(this, wk.p, l, shares, ids, np, item_stride, nitems, nchunks, dimension, status,
                                             errpos, summary, st);
  }
  // the in-mask rows of a list for up to three compact words [np][width], item_stride apart, in one launch: row r of item y
  // becomes x * k (with `scale`) + row ids[r] of masks[y]; a null mask skips the item (vec_add_list_rows_kernel, ntt.hpp)
  int add_list_rows(Fr* x, size_t item_stride, const Fr* const* masks, int items, const uint32_t* ids, int np, bool scale,
                    const Fr& k, size_t width, hipStream_t st) {
    ListMasks<Fr> lm{};
    bool any = false;
    for (int y = 0; y < items && y < 3; y++) any = (lm.mask[y] = masks[y]) || any;
    if (!any || !width) return ZK_OK;
    uint32_t listed = 0;
    for (int i = 0; i < np; i++) listed |= 1u << ids[i];
    const size_t cnt = width * (size_t)np;
    vec_add_list_rows_kernel<Fr><<<dim3((unsigned)((cnt + 255) / 256), (unsigned)items), dim3(256), 0, st>>>(
        x, item_stride, lm, listed, scale ? 1 : 0, k, width, (size_t)np);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
  }

  // ---------------------------------------------------------------- checked king rounds (all n parties)
  // Each repairs the word the king receives, then runs the unchecked king launch on the repaired matrix.  A failed chunk is
  // no error return: its shares go to the king as received and the caller reads summary[2].
  // king of d_fft / d_ifft (dfft/mod.rs:264-304): the word is `in` itself, degree < 2l, so up to l wrong shares per chunk
  int fft2_king_checked(void* in, const uint32_t* parties, int np, int log_m, int inverse, const void* g, int scale_size_inv,
                        int rearrange, uint64_t seed, void* out, const void* out_mask, uint8_t* status, uint32_t* errpos,
                        uint64_t* summary, hipStream_t st) override {
    (void)parties;
    if (np != n)
      return fail(ZK_ERR_BAD_INPUT, "the checked king takes all n parties: a party list is the unchecked zk_fft2_king's");
    if (!in || !out) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (log_m < ilog2(l)) return fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT");
    int rc = pss_repair(in, ((size_t)1 << log_m) / l, 2 * l, status, errpos, summary, st);
    if (rc) return rc;
    return fft2_king(in, nullptr, nullptr, n, log_m, inverse, g, scale_size_inv, rearrange, seed, out, out_mask, st);
  }
  // d_fft / d_ifft: the word checked is what the reference's king receives, fft1(x) + in_mask, for the inverse
  // fft1(x) / m + in_mask (dfft/mod.rs:159, :254-258).  It is materialised in the stream's king_tmp -- the mask through the
  // last pass of fft1, after a scaling pass of its own for the inverse -- so the king runs with no in-mask and, where the 1 / m
  // is already in the word, no second scaling.  Without a mask the inverse's word is fft1(x): a multiple of a codeword is one,
  // and the king folds 1 / m into its g^i table as the unchecked call does.
  int d_fft_checked(void* shares, const void* in_mask, const void* out_mask, int rearrange, int log_m, int inverse,
                    const void* g, uint64_t seed, void* out, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                    hipStream_t st) override {
    if (!shares) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (out == shares) out = nullptr;
    const int log_l = ilog2(l);
    if (log_m < log_l) return fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT");
    const size_t Lc = ((size_t)1 << log_m) / l, cnt = (size_t)n * Lc;
    DevBuf& king_tmp_ = ws(st)->king_tmp;
    ZK_HIP(king_tmp_.ensure(cnt * sizeof(Fr)));
    NttSrc<Fr> src{};
    src.p[0] = (const Fr*)shares;
    src.per = (uint32_t)n;
    const bool scaled = inverse && in_mask;
    int rc = fft1_src(king_tmp_.p, log_m, inverse, (size_t)n, scaled ? nullptr : in_mask, st, src);
    if (rc) return rc;
    if (scaled) {
      const Fr minv = Fr::from_u64((uint64_t)1 << log_m).inverse();      // as the masked d_ifft of engine_dist.inc.hpp
      if ((rc = vec_scale(king_tmp_.p, &minv, cnt, st))) return rc;
      if ((rc = vec_add(king_tmp_.p, in_mask, cnt, st))) return rc;
    }
    if ((rc = pss_repair(king_tmp_.p, Lc, 2 * l, status, errpos, summary, st))) return rc;
    return fft2_king(king_tmp_.p, nullptr, nullptr, n, log_m, inverse, g, inverse && !scaled ? 1 : 0, rearrange, seed,
                     out ? out : shares, out_mask, st);
  }
  // deg_red (deg_red.rs:99-115): the word is x + in_mask, added into x (the call is in place), of degree <= 4l - 2.  At
  // dimension 4l - 1 the cap is 0: DETECTION ONLY -- a status is 0 or 2, errpos is 0 and nothing is ever rewritten.
  int deg_red_checked(void* x, const void* in_mask, const void* out_mask, size_t len, uint64_t seed, uint8_t* status,
                      uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    // what pss_repair would refuse is refused before the mask is added: a bad-input return leaves x as it was
    if (len && (!x || !status)) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (len >= ((size_t)1 << 32)) return fail(ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks");
    int rc;
    if (in_mask && (rc = vec_add(x, in_mask, (size_t)n * len, st))) return rc;
    if ((rc = pss_repair(x, len, 4 * l - 1, status, errpos, summary, st))) return rc;
    return deg_red_np((const Fr*)x, nullptr, nullptr, n, len, seed, (Fr*)x, (const Fr*)out_mask, st);
  }

  // ---------------------------------------------------------------- zk_pss_repair_parties
  // shares [nparties][nchunks] of the listed parties, in place: status, errpos and summary are pss_unpack_robust_parties'; in a
  // corrected chunk the element in the row of every listed party named in errpos becomes h(w_n^p), every other element keeps
  // its bytes.  With nparties == n this is pss_repair.
  int pss_repair_parties(void* shares, const uint32_t* parties, int nparties, size_t nchunks, int dimension, uint8_t* status,
                         uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    return gao_repair_parties_run<FrP>(this, ws(st)->hwork, l, shares, parties, nparties, nchunks, dimension, status, errpos,
                                       summary, st);
  }

  // ---------------------------------------------------------------- the range form of zk_pss_repair_parties
  // The word of an all-to-all king (engine_dist.inc.hpp): rg.cnt valid columns of a block [nparties][rg.stride], column c
  // being chunk rg.chunk(c) of a word of rg.len chunks (king_range.hpp).  Only those columns are read and rewritten, status
  // and errpos [rg.len] are written at the mapped chunks only, the summary counts the rg.cnt chunks.
  int pss_repair_range(void* shares, const uint32_t* parties, int nparties, size_t stride, uint32_t cnt, uint32_t len,
                       uint32_t base, uint32_t shift, int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                       hipStream_t st) override {
    const GaoRange rg{stride, cnt, base, shift, len};
    return gao_repair_range_run<FrP>(this, ws(st)->hwork, l, shares, parties, nparties, rg, dimension, status, errpos, summary,
                                     st);
  }

  // ---------------------------------------------------------------- checked king rounds with a party list
  // Only the listed parties' words reached the king: repair with the list at dimension 2l, cap = (np - 2l) / 2, then the
  // unchecked king with the same list (umat_for).  The refusals are pss_repair_parties' and the unchecked king's (checked_list).
  // deg_red has no such form: at dimension 4l - 1 a list of n - 1 parties has no redundancy left.
  int fft2_king_checked_parties(void* in, const uint32_t* parties, int np, int log_m, int inverse, const void* g,
                                int scale_size_inv, int rearrange, uint64_t seed, void* out, const void* out_mask,
                                uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    if (!in || !out) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (log_m < ilog2(l)) return fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT");
    uint32_t ids[GAO_MAX_N];
    int rc = checked_list(parties, np, 2 * l, ids);
    if (rc) return rc;
    if ((rc = pss_repair_parties(in, ids, np, ((size_t)1 << log_m) / l, 2 * l, status, errpos, summary, st))) return rc;
    return fft2_king(in, nullptr, ids, np, log_m, inverse, g, scale_size_inv, rearrange, seed, out, out_mask, st);
  }
  // the list as pss_repair_parties reads it, refused as it refuses it, and as the king's umat_for refuses it: the reference's
  // unpack_missing_shares takes a list only with more than 2 (t + l - 1) = 4l - 2 shares (pss.rs:183-186), so a list is all n
  // parties or n - 1 of them.  Asked before anything is written: a refusal leaves the caller's buffers as they were.
  int checked_list(const uint32_t* parties, int np, int dimension, uint32_t* ids) {
    if (np <= 0 || np > n) return fail(ZK_ERR_BAD_INPUT, "bad party count");
    for (int i = 0; i < np; i++) {
      ids[i] = parties ? parties[i] : (uint32_t)i;
      if (ids[i] >= (uint32_t)n || (i > 0 && ids[i] <= ids[i - 1]))
        return fail(ZK_ERR_BAD_INPUT, "party ids must be ascending and < n");
    }
    if (np <= dimension || (np < n && np <= 4 * l - 2))
      return fail(ZK_ERR_PROTOCOL, "Not enough shares to reconstruct");      // pss.rs:183-186
    return ZK_OK;
  }
  // d_fft / d_ifft: shares, in_mask and the outputs are [n][m/l]; the king's word is compact, [np][m/l] in king_tmp: row i is
  // fft1 of the row of parties[i] (NttSrc with one vector per pointer), for the inverse times 1 / m, plus that party's in-mask
  // row -- built as d_fft_checked builds its word, row by row.
  int d_fft_checked_parties(void* shares, const uint32_t* parties, int np, const void* in_mask, const void* out_mask,
                            int rearrange, int log_m, int inverse, const void* g, uint64_t seed, void* out, uint8_t* status,
                            uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    if (!shares) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (out == shares) out = nullptr;
    const int log_l = ilog2(l);
    if (log_m < log_l) return fail(ZK_ERR_BAD_INPUT, "Mismatch of size in FFT");
    uint32_t ids[GAO_MAX_N];
    int rc = checked_list(parties, np, 2 * l, ids);
    if (rc) return rc;
    if (np == n) return d_fft_checked(shares, in_mask, out_mask, rearrange, log_m, inverse, g, seed, out, status, errpos,
                                      summary, st);
    const size_t Lc = ((size_t)1 << log_m) / l, cnt = (size_t)np * Lc;
    DevBuf& king_tmp_ = ws(st)->king_tmp;
    ZK_HIP(king_tmp_.ensure(cnt * sizeof(Fr)));
    Fr* word = (Fr*)king_tmp_.p;
    const bool scaled = inverse && in_mask;
    const Fr minv = scaled ? Fr::from_u64((uint64_t)1 << log_m).inverse() : Fr::one();
    static_assert(GAO_MAX_N <= NTT_SRC_MAX, "one pointer per listed row");
    NttSrc<Fr> src{};
    for (int i = 0; i < np; i++) src.p[i] = (const Fr*)shares + (size_t)ids[i] * Lc;
    src.per = 1;
    // (a mask folded into fft1's last pass is one contiguous [batch][m/l] vector: the rows of a list are not, they are added below)
    if ((rc = fft1_src(word, log_m, inverse, (size_t)np, nullptr, st, src))) return rc;
    if (scaled && (rc = vec_scale(word, &minv, cnt, st))) return rc;
    if (in_mask)
      for (int i = 0; i < np; i++)
        if ((rc = vec_add(word + (size_t)i * Lc, (const Fr*)in_mask + (size_t)ids[i] * Lc, Lc, st))) return rc;
    if ((rc = pss_repair_parties(word, ids, np, Lc, 2 * l, status, errpos, summary, st))) return rc;
    return fft2_king(word, nullptr, ids, np, log_m, inverse, g, inverse && !scaled ? 1 : 0, rearrange, seed,
                     out ? out : shares, out_mask, st);
  }
  // d_pp (dpp/mod.rs:37-52): the king's word is num ++ den per party, packed shares of degree < 2l; two repairs, then the
  // unchecked king with the list.  status / errpos [2 len], summary [2][3 + n]: num's, then den's.  The deg_red that ends
  // d_pp is not checked: the king produced that word itself and its cap is 0.
  int d_pp_checked(void* num, void* den, const uint32_t* parties, int np, const void* in_mask, const void* out_mask, size_t len,
                   uint64_t seed, void* out, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    uint32_t ids[GAO_MAX_N];
    int rc = checked_list(parties, np, 2 * l, ids);
    if (rc) return rc;
    if (!len) return ZK_OK;
    if (!num || !den || !out || !status) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (len >= ((size_t)1 << 31)) return fail(ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks");
    if ((rc = pss_repair_parties(num, ids, np, len, 2 * l, status, errpos, summary, st))) return rc;
    if ((rc = pss_repair_parties(den, ids, np, len, 2 * l, status + len, errpos ? errpos + len : nullptr,
                                 summary ? summary + 3 + n : nullptr, st)))
      return rc;
    return d_pp_king((const Fr*)num, (const Fr*)den, ids, np, len, seed, (Fr*)out, st, true, (const Fr*)in_mask,
                     (const Fr*)out_mask);
  }
