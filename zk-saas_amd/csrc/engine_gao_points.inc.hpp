// Part of class Engine<Cfg> (engine_impl.hpp includes this file INSIDE the class body): zk_pss_unpack_points_robust and
// zk_pss_repair_points, the robust unpack of packed point shares and its repair form, and zk_d_msm_checked.  Kernels and
// driver: gao_points_impl.hpp, compiled in gao_points_<curve>.hip.  Not a stand-alone header.

  // ---------------------------------------------------------------- zk_pss_unpack_points_robust / zk_pss_repair_points
  // shares [n][nchunks] affine of all n parties.  The secrets go through the matrix of the plain call: unpack's (U1) up to
  // dimension 2l, unpack2's (U2) above, the canonical device copies zk_pss_unpack_points caches.  Working memory is the
  // caller stream's hwork; no host synchronisation once that matrix and the decoder's table are cached.
  // the decoder's scalars (GaoPtTable: they depend on l only), built and uploaded once per context, as the unpack matrix is
  GaoPtTable<Fr>* gao_pt_tab_ = nullptr;
  int gao_points_table(const GaoPtTable<Fr>** out) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!gao_pt_tab_) {
      const GaoPtTable<Fr> t = gao_points_make_table<FrP>(l);
      GaoPtTable<Fr>* d = nullptr;
      ZK_HIP(hipMalloc((void**)&d, sizeof(t)));
      ZK_HIP(hipMemcpy(d, &t, sizeof(t), hipMemcpyHostToDevice));
      gao_pt_tab_ = d;
    }
    *out = gao_pt_tab_;
    return ZK_OK;
  }
  template <class Fld, bool REPAIR>
  int points_robust_t(std::conditional_t<REPAIR, void*, const void*> shares, size_t nchunks, int dimension, void* out,
                      uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) {
    Fr* Ud = nullptr;
    if (!REPAIR && out && nchunks) {
      int rc = ucanon_for(nullptr, n, dimension <= 2 * l ? 1 : 2, &Ud);
      if (rc) return rc;
    }
    const GaoPtTable<Fr>* tab = nullptr;
    if (nchunks) {
      int rc = gao_points_table(&tab);
      if (rc) return rc;
    }
    return gao_points_run<FrP, Fld, REPAIR>(this, ws(st)->hwork, l, shares, nchunks, dimension, tab, Ud, nullptr, out, status,
                                            errpos, summary, st);
  }
  int pss_unpack_points_robust(int group, const void* shares, size_t nchunks, int dimension, void* out, uint8_t* status,
                               uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    if (group == ZK_G1) return points_robust_t<Fq_, false>(shares, nchunks, dimension, out, status, errpos, summary, st);
    if (group == ZK_G2) {
      if constexpr (Cfg::HAS_G2)
        return points_robust_t<Fq2_, false>(shares, nchunks, dimension, out, status, errpos, summary, st);
    }
    return fail(ZK_ERR_BAD_INPUT, "bad group");
  }
  int pss_repair_points(int group, void* shares, size_t nchunks, int dimension, uint8_t* status, uint32_t* errpos,
                        uint64_t* summary, hipStream_t st) override {
    if (group == ZK_G1) return points_robust_t<Fq_, true>(shares, nchunks, dimension, nullptr, status, errpos, summary, st);
    if (group == ZK_G2) {
      if constexpr (Cfg::HAS_G2)
        return points_robust_t<Fq2_, true>(shares, nchunks, dimension, nullptr, status, errpos, summary, st);
    }
    return fail(ZK_ERR_BAD_INPUT, "bad group");
  }

  // ---------------------------------------------------------------- the same with a party list
  // shares [np][nchunks] affine of the listed parties.  The list's table (gao_points_make_list: syndrome rows, error scalars,
  // rows, the Lagrange matrix) depends on (party mask, dimension) only: built on the host per call, its device copy cached
  // like the unpack matrices.  The refusals, in the order the header gives them.
  std::map<uint64_t, std::pair<void*, GaoPtList<Fr>>> gao_pt_lists_;
  int gao_points_list(const uint32_t* parties, int np, int dimension, GaoPtList<Fr>* out) {
    uint32_t mask = 0;
    for (int i = 0; i < np; i++) mask |= 1u << (parties ? parties[i] : (uint32_t)i);
    const uint64_t key = ((uint64_t)dimension << 32) | mask;
    std::lock_guard<std::mutex> lk(mu_);
    auto it = gao_pt_lists_.find(key);
    if (it == gao_pt_lists_.end()) {
      const GaoPtListHost<Fr> t = gao_points_make_list<FrP>(l, parties, np, dimension);
      std::vector<char> img(t.bytes());
      memcpy(img.data(), t.row, GAO_PT_LIST_HEAD);
      memcpy(img.data() + GAO_PT_LIST_HEAD, t.sc.data(), t.sc.size() * sizeof(Fr));
      void* d = nullptr;
      ZK_HIP(hipMalloc(&d, img.size()));
      hipError_t err = hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice);
      if (err != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(err, "hipMemcpy(party list table)");
      }
      it = gao_pt_lists_.emplace(key, std::make_pair(d, t.view(d))).first;
    }
    *out = it->second.second;
    return ZK_OK;
  }
  // the count and the ids of gao_list_check; the dimension and too few shares are refused below, behind other refusals and
  // with the party 0
  int points_party_list_ok(const uint32_t* parties, int np) {
    uint32_t ids[GAO_MAX_N];
    return refuse(gao_list_check(parties, np, 0, n, ids, true));
  }
  template <bool REPAIR>
  int points_robust_parties(int group, std::conditional_t<REPAIR, void*, const void*> shares, const uint32_t* parties, int np,
                            size_t nchunks, int dimension, void* out, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                            hipStream_t st) {
    int rc = points_party_list_ok(parties, np);
    if (rc) return rc;
    if (dimension < 1 || dimension > n - 1) return fail(ZK_ERR_BAD_INPUT, "dimension must lie in 1 .. n - 1");
    if (group != ZK_G1 && !(group == ZK_G2 && Cfg::HAS_G2)) return fail(ZK_ERR_BAD_INPUT, "bad group");
    if (nchunks && (!shares || !status)) return fail(ZK_ERR_BAD_INPUT, "null pointer");
    if (np <= dimension) return fail(ZK_ERR_PROTOCOL, "Not enough shares for this dimension", 0);
    if (nchunks == 0) return ZK_OK;
    GaoPtList<Fr> lt;
    rc = gao_points_list(parties, np, dimension, &lt);
    if (rc) return rc;
    const GaoPtTable<Fr>* tab = nullptr;
    rc = gao_points_table(&tab);
    if (rc) return rc;
    return msm_.by_group(this, group, [&](auto fld) {
      using Fld = decltype(fld);
      return gao_points_run<FrP, Fld, REPAIR>(this, ws(st)->hwork, l, shares, nchunks, dimension, tab, nullptr, &lt, out, status,
                                              errpos, summary, st);
    });
  }
  int pss_unpack_points_robust_parties(int group, const void* shares, const uint32_t* parties, int np, size_t nchunks,
                                       int dimension, void* out, uint8_t* status, uint32_t* errpos, uint64_t* summary,
                                       hipStream_t st) override {
    return points_robust_parties<false>(group, shares, parties, np, nchunks, dimension, out, status, errpos, summary, st);
  }
  int pss_repair_points_parties(int group, void* shares, const uint32_t* parties, int np, size_t nchunks, int dimension,
                                uint8_t* status, uint32_t* errpos, uint64_t* summary, hipStream_t st) override {
    return points_robust_parties<true>(group, shares, parties, np, nchunks, dimension, nullptr, status, errpos, summary, st);
  }

  // ---------------------------------------------------------------- zk_groth16_reconstruct_robust
  // r and s are in the clear in this project, so a party's shares of A, B and C are fixed linear combinations
  // of d_msm outputs and clear points: words of dimension 2l, which leaves np - 2l syndromes.  Chunk = proof: the shares are
  // copied up once, staged as the compact affine [np][nproofs] of each element, tested with the subgroup predicate (a share
  // that fails becomes the identity: an ordinary wrong share from there on), and decoded by three calls of the party-list
  // unpack; secret 0 of a chunk is the element.  The bytes go through the device codec in zk_groth16_reconstruct's order.
  DevBuf recon_robust_;
  int groth16_reconstruct_robust(size_t nproofs, const void* pi_a, const void* pi_b, const void* pi_c, const uint32_t* parties,
                                 int np, void* proofs_affine, void* proofs_bytes, uint8_t* status, uint32_t* errpos,
                                 const SubgroupCheckFn& subgroup, hipStream_t st) override {
    if constexpr (!Cfg::HAS_G2) {
      return fail(ZK_ERR_BAD_INPUT, "G2 is not available for this curve");
    } else {
      using A1 = Affine<Fq_>;
      using A2 = Affine<Fq2_>;
      int rc = points_party_list_ok(parties, np);
      if (rc) return rc;
      if (!status) return fail(ZK_ERR_BAD_INPUT, "null status");
      if (np <= 2 * l) return fail(ZK_ERR_PROTOCOL, "Not enough shares to reconstruct", 0);
      if (nproofs == 0) return ZK_OK;
      if (!pi_a || !pi_b || !pi_c) return fail(ZK_ERR_BAD_INPUT, "null pointer");
      if (nproofs >= ((size_t)1 << 32) / (size_t)n) return fail(ZK_ERR_BAD_INPUT, "too many proofs");
      constexpr size_t NB = (Cfg::FqP::BITS + 7) / 8;
      const size_t cnt = nproofs * (size_t)np;
      size_t bytes = 0;
      auto take = [&](size_t b) {
        const size_t o = bytes;
        bytes += (b + 255) / 256 * 256;
        return o;
      };
      const size_t o_jac = take(cnt * sizeof(Jacobian<Fq2_>)), o_sh = take(cnt * sizeof(A2)), o_ok = take(cnt);
      const size_t o_out = take(nproofs * (size_t)l * sizeof(A2));
      const size_t o_st = take(3 * nproofs), o_ep = take(3 * nproofs * sizeof(uint32_t));
      const size_t o_g1 = take(2 * nproofs * sizeof(A1)), o_g2 = take(nproofs * sizeof(A2)), o_by = take(4 * nproofs * NB);
      ZK_HIP(recon_robust_.ensure(bytes));
      char* d = (char*)recon_robust_.p;
      uint8_t* st_d = (uint8_t*)(d + o_st);
      uint32_t* ep_d = (uint32_t*)(d + o_ep);
      // element e (0 A, 1 B, 2 C) of every proof -> dst[nproofs] affine; the staging buffers serve one element after the other
      auto element = [&](auto tag, int group, int e, const void* jac, void* dst) {
        using Fld = decltype(tag);
        using A = Affine<Fld>;
        ZK_HIP(hipMemcpyAsync(d + o_jac, jac, cnt * sizeof(Jacobian<Fld>), hipMemcpyHostToDevice, st));
        const dim3 grid((unsigned)((cnt + 127) / 128)), blk(128);
        points_stage_shares_kernel<Fld><<<grid, blk, 0, st>>>((const Jacobian<Fld>*)(d + o_jac), nproofs, np, (A*)(d + o_sh));
        ZK_HIP(hipGetLastError());
        int rc2 = subgroup(group, d + o_sh, cnt, (uint8_t*)(d + o_ok));
        if (rc2) return rc2;
        points_drop_failed_kernel<Fld><<<grid, blk, 0, st>>>((A*)(d + o_sh), (const uint8_t*)(d + o_ok), cnt);
        ZK_HIP(hipGetLastError());
        rc2 = points_robust_parties<false>(group, d + o_sh, parties, np, nproofs, 2 * l, d + o_out, st_d + e * nproofs,
                                           ep_d + e * nproofs, nullptr, st);
        if (rc2) return rc2;
        ZK_HIP(hipMemcpy2DAsync(dst, sizeof(A), d + o_out, (size_t)l * sizeof(A), sizeof(A), nproofs, hipMemcpyDeviceToDevice,
                                st));                                                 // secret 0 of each chunk
        return (int)ZK_OK;
      };
      A1* g1s = (A1*)(d + o_g1);                                                       // A of every proof, then C
      rc = element(Fq_{}, ZK_G1, 0, pi_a, g1s);
      if (rc) return rc;
      rc = element(Fq2_{}, ZK_G2, 1, pi_b, d + o_g2);
      if (rc) return rc;
      rc = element(Fq_{}, ZK_G1, 2, pi_c, g1s + nproofs);
      if (rc) return rc;
      char* bytes_d = d + o_by;
      if (proofs_bytes) {
        rc = points_codec_t<Fq_>(g1s, 2 * nproofs, bytes_d, 0, Fq_::zero(), st);                      // a, c -> [0, 2 NB nproofs)
        if (rc) return rc;
        rc = points_codec_t<Fq2_>(d + o_g2, nproofs, bytes_d + 2 * nproofs * NB, 0, Fq2_{}, st);      // b after them
        if (rc) return rc;
      }
      std::vector<uint8_t> hst(3 * nproofs), hb(proofs_bytes ? 4 * nproofs * NB : 0);
      std::vector<uint32_t> hep(3 * nproofs);
      std::vector<A1> h1(proofs_affine ? 2 * nproofs : 0);
      std::vector<A2> h2(proofs_affine ? nproofs : 0);
      ZK_HIP(hipMemcpyAsync(hst.data(), st_d, hst.size(), hipMemcpyDeviceToHost, st));
      ZK_HIP(hipMemcpyAsync(hep.data(), ep_d, hep.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      if (proofs_affine) {
        ZK_HIP(hipMemcpyAsync(h1.data(), g1s, h1.size() * sizeof(A1), hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(h2.data(), d + o_g2, h2.size() * sizeof(A2), hipMemcpyDeviceToHost, st));
      }
      if (proofs_bytes) ZK_HIP(hipMemcpyAsync(hb.data(), bytes_d, hb.size(), hipMemcpyDeviceToHost, st));
      ZK_HIP(hipStreamSynchronize(st));
      for (size_t i = 0; i < nproofs; i++) {
        bool failed = false;
        for (int e = 0; e < 3; e++) {
          status[3 * i + e] = hst[e * nproofs + i];
          if (errpos) errpos[3 * i + e] = hep[e * nproofs + i];
          failed = failed || hst[e * nproofs + i] == 2;
        }
        if (proofs_affine) {                              // a failed element is the identity the decoder wrote: (0, 0)
          char* o = (char*)proofs_affine + i * 4 * sizeof(A1);
          memcpy(o, &h1[i], sizeof(A1));
          memcpy(o + sizeof(A1), &h2[i], sizeof(A2));
          memcpy(o + sizeof(A1) + sizeof(A2), &h1[nproofs + i], sizeof(A1));
        }
        if (proofs_bytes) {
          uint8_t* ob = (uint8_t*)proofs_bytes + i * 4 * NB;
          if (failed) {
            memset(ob, 0, 4 * NB);
          } else {
            memcpy(ob, hb.data() + i * NB, NB);                                        // a
            memcpy(ob + NB, hb.data() + 2 * nproofs * NB + i * 2 * NB, 2 * NB);        // b
            memcpy(ob + 3 * NB, hb.data() + (nproofs + i) * NB, NB);                   // c
          }
        }
      }
      return ZK_OK;
    }
  }

  // ---------------------------------------------------------------- zk_d_msm_checked
  // The king's word c_p = msm_p + in_mask_p (dmsm/mod.rs:73-85) has degree <= 4l - 2: dimension 4l - 1, one syndrome,
  // sum_p w_n^p c_p (n times the top coefficient of the interpolant), detection only.  It is a second fused MSM with the
  // coefficients w_n^p in place of coef_p -- the route of a party list, d_msm_coef_t -- whose king value lands in a scratch
  // row of n points.  No MSM kernel, plan or sort is touched; `out` is d_msm's, written first.
  int d_msm_checked(int group, const void* bases, const void* scalars, size_t len, const void* in_mask, const void* out_mask,
                    void* out, uint8_t* status, hipStream_t st) override {
    if (!status) return fail(ZK_ERR_BAD_INPUT, "null status");
    if (group != ZK_G1 && !(group == ZK_G2 && Cfg::HAS_G2)) return fail(ZK_ERR_BAD_INPUT, "bad group");
    int rc = d_msm(group, bases, scalars, len, in_mask, out_mask, out, st);
    if (rc) return rc;
    std::vector<Fr> x, y, z;
    points(x, y, z);
    const std::vector<Fr> coef(x.begin(), x.begin() + n);       // x_p = w_n^p
    return msm_.by_group(this, group, [&](auto fld) {
      using Fld = decltype(fld);
      std::vector<Jacobian<Fld>> king((size_t)n);
      int rc2 = msm_.template d_msm_coef_t<Fld>(this, bases, scalars, len, coef, in_mask, nullptr, king.data(), st);
      if (!rc2) *status = king[0].Z.is_zero() ? 0 : 2;
      return rc2;
    });
  }
