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
    return gao_points_run<FrP, Fld, REPAIR>(this, ws(st)->hwork, l, shares, nchunks, dimension, tab, Ud, out, status, errpos,
                                            summary, st);
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
