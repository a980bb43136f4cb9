// Part of class Engine<Cfg> (engine_impl.hpp includes this file INSIDE the class body): zk_pss_unpack_robust and
// zk_pss_unpack_robust_parties, the error-correcting unpack.  Kernels and driver: gao_impl.hpp, compiled in gao_<curve>.hip.  Not a stand-alone header.

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
