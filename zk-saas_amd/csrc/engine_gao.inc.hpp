// Part of class Engine<Cfg> (engine_impl.hpp includes this file INSIDE the class body): zk_pss_unpack_robust and
// zk_pss_unpack_robust_parties, the error-correcting unpack; zk_pss_repair and the checked king rounds built on it.  Kernels and driver: gao_impl.hpp, compiled in gao_<curve>.hip.  Not a stand-alone header.

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
