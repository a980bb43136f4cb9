// Part of class Engine<Cfg> (engine_impl.hpp includes this file INSIDE the class body): the error-correcting unpack and the
// repair of packed scalar shares -- every zk_pss_unpack_robust* and zk_pss_repair* entry point builds a GaoCall (gao.hpp) for
// the one driver gao_run (gao_impl.hpp, compiled in gao_<curve>.hip) -- and the checked king rounds built on them.  Not a
// stand-alone header.

  // a refusal of gao.hpp's host checks as this context's error
  int refuse(const GaoRefusal& r) { return r.code ? fail(r.code, r.msg) : (int)ZK_OK; }
  // One word (or one word in a range): working memory is the caller stream's hwork (StreamWs), sized here; no host
  // synchronisation.  A call gao_run will refuse, or one of no chunks, needs none.
  template <bool REPAIR>
  int gao_word(const GaoCall& c, hipStream_t st) {
    DevBuf& wk = ws(st)->hwork;
    uint32_t ids[GAO_MAX_N];
    if (c.nchunks && !gao_call_check(l, c, REPAIR, ids).code)
      ZK_HIP(wk.ensure(gao_layout<Fr>(n, 1, c.nchunks, c.np < n, REPAIR).bytes));
    return gao_run<FrP, REPAIR>(this, wk.p, l, c, st);
  }
  static GaoCall gao_call(const void* shares, const uint32_t* parties, int np, size_t nchunks, int dimension, uint8_t* status,
                          uint32_t* errpos, uint64_t* summary) {
    GaoCall c;
    c.shares = const_cast<void*>(shares), c.ids = parties, c.np = np, c.nchunks = nchunks, c.dimension = dimension;
    c.status = status, c.errpos = errpos, c.summary = summary;
    return c;
  }

  // ---------------------------------------------------------------- zk_pss_unpack_robust, zk_pss_unpack_robust_parties
  // shares [nparties][nchunks] of the listed parties (ascending ids; null: 0 .. nparties - 1), all n of them in the first
  // form; any of secrets, message, errpos, summary may be null.
  int pss_unpack_robust(const void* shares, size_t nchunks, int dimension, void* secrets, void* message, uint8_t* status,
                        uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    return pss_unpack_robust_parties(shares, nullptr, n, nchunks, dimension, secrets, message, status, errpos, summary, st);
  }
  int pss_unpack_robust_parties(const void* shares, const uint32_t* parties, int nparties, size_t nchunks, int dimension,
                                void* secrets, void* message, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                                hipStream_t st) override {
    GaoCall c = gao_call(shares, parties, nparties, nchunks, dimension, status, errpos, summary);
    c.secrets = secrets, c.message = message;
    return gao_word<false>(c, st);
  }

  // ---------------------------------------------------------------- zk_pss_repair, zk_pss_repair_parties
  // shares [nparties][nchunks] of the listed parties, in place: status, errpos and summary are the unpack's; in a corrected
  // chunk the element in the row of every listed party named in errpos becomes h(w_n^p), every other element keeps its bytes.
  int pss_repair(void* shares, size_t nchunks, int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                 hipStream_t st) override {
    return pss_repair_parties(shares, nullptr, n, nchunks, dimension, status, errpos, summary, st);
  }
  int pss_repair_parties(void* shares, const uint32_t* parties, int nparties, size_t nchunks, int dimension, uint8_t* status,
                         uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    return gao_word<true>(gao_call(shares, parties, nparties, nchunks, dimension, status, errpos, summary), st);
  }

  // ---------------------------------------------------------------- the range form of zk_pss_repair_parties
  // The word of an all-to-all king (engine_dist.inc.hpp): rg.cnt valid columns of a block [nparties][rg.stride], column c
  // being chunk rg.chunk(c) of a word of rg.len chunks (king_range.hpp).  Only those columns are read and rewritten, status
  // and errpos [rg.len] are written at the mapped chunks only, the summary counts the rg.cnt chunks.
  int pss_repair_range(void* shares, const uint32_t* parties, int nparties, size_t stride, uint32_t cnt, uint32_t len,
                       uint32_t base, uint32_t shift, int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                       hipStream_t st) override {
    const GaoRange rg{stride, cnt, base, shift, len};
    GaoCall c = gao_call(shares, parties, nparties, cnt, dimension, status, errpos, summary);
    c.range = &rg;
    return gao_word<true>(c, st);
  }

  // ---------------------------------------------------------------- zk_pss_repair_batch, zk_pss_repair_batch_parties
  // nitems matrices [nparties][nchunks] of ONE party list (all n parties in the first form), item i at shares + i * item_stride
  // (KingBatch::stride; circom_h's W0 / W1): the repair of each, with ONE clear, the tables of the list put into working
  // memory once, ONE scan launch (the item on grid.y) and ONE decoder launch over one list of dirty (item, chunk) entries.
  // status / errpos [nitems][nchunks], summary [nitems][3 + n].  A refusal writes nothing.
  static_assert(GAO_BATCH_MAX == KING_BATCH, "a repair batch takes the items of a king batch");
  // The refusals of a batch.  list_first: zk_pss_repair_batch_parties refuses its list, dimension and too few shares ahead of
  // a bad item count, zk_pss_repair_batch a bad item count ahead of the dimension.
  int repair_batch_check(const GaoCall& c, bool list_first, uint32_t* ids) {
    int rc;
    if (list_first && (rc = refuse(gao_list_check(c.ids, c.np, c.dimension, n, ids)))) return rc;
    if (c.nitems < 1 || c.nitems > KING_BATCH) return fail(ZK_ERR_BAD_INPUT, "bad repair batch");
    if (!list_first && (rc = refuse(gao_list_check(c.ids, c.np, c.dimension, n, ids)))) return rc;
    if (c.nchunks == 0) return ZK_OK;
    if (!c.shares || !c.status) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (!gao_batch_fits((uint64_t)c.nitems, c.nchunks)) return fail(ZK_ERR_BAD_INPUT, "more than 2^32 - 1 chunks in the batch");
    if (c.item_stride < (size_t)c.np * c.nchunks)
      return fail(ZK_ERR_BAD_INPUT, c.np == n ? "item stride below n * nchunks" : "item stride below nparties * nchunks");
    return ZK_OK;
  }
  int repair_batch(const uint32_t* parties, int np, bool list_first, void* shares, size_t item_stride, int nitems, size_t nchunks,
                   int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) {
    GaoCall c = gao_call(shares, parties, np, nchunks, dimension, status, errpos, summary);
    c.nitems = nitems, c.item_stride = item_stride;
    uint32_t ids[GAO_MAX_N];
    int rc = repair_batch_check(c, list_first, ids);
    if (rc || !nchunks) return rc;
    DevBuf& wk = ws(st)->hwork;
    ZK_HIP(wk.ensure(gao_layout<Fr>(n, nitems, nchunks, np < n).bytes));
    return gao_run<FrP, true>(this, wk.p, l, c, st);
  }
  int pss_repair_batch(void* shares, size_t item_stride, int nitems, size_t nchunks, int dimension, uint8_t* status,
                       uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    return repair_batch(nullptr, n, false, shares, item_stride, nitems, nchunks, dimension, status, errpos, summary, st);
  }
  int pss_repair_batch_parties(void* shares, const uint32_t* parties, int np, size_t item_stride, int nitems, size_t nchunks,
                               int dimension, uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    return repair_batch(parties, np, true, shares, item_stride, nitems, nchunks, dimension, status, errpos, summary, st);
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
    int rc = refuse(gao_list_check(parties, np, dimension, n, ids));
    if (rc) return rc;
    if (np < n && np <= 4 * l - 2) return fail(ZK_ERR_PROTOCOL, "Not enough shares to reconstruct");      // pss.rs:183-186
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
