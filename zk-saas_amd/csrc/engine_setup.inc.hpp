// Part of class Engine<Cfg> (engine_impl.hpp includes this file INSIDE the class body): zk_groth16_setup_scalars, the
// circuit-specific setup in the exponent.  Kernels and driver: setup_impl.hpp, compiled in setup_<curve>.hip.  Not a
// stand-alone header.

  // ---------------------------------------------------------------- zk_groth16_setup_scalars
  // mats = A, B, C as {row_ptr, col, val}; out = a_query, b_query, l_query, h_query, gamma_abc.  Working memory is the
  // caller stream's hwork (StreamWs).
  int groth16_setup_scalars(const void* const mats[9], size_t nvars, size_t nc, size_t ni, int log_m, const void* trapdoor,
                            size_t tail, void* const out[5], hipStream_t st) override {
    return setup_scalars_run<FrP>(this, ws(st)->hwork, mats, nvars, nc, ni, log_m, trapdoor, tail, out, st);
  }
