// Groth16 circuit-specific setup in the exponent (ark_groth16::generate_parameters with the circom reduction): R1CS and
// trapdoor -> the discrete logs of the CRS vectors, on the device (zk_groth16_setup_scalars).  Three parts:
//   (a) quotient vectors: out_i = num_i / den_i with a batch inversion per lane -- the Lagrange coefficients of the size-m
//       domain at tau and h_query in closed form;
//   (b) the transposed sparse products A^T u, B^T u, C^T u from row-CSR: column histogram, exclusive scan, scatter of
//       (row, nonzero) pairs into column order, then a gather per column -- one lane for a short column, workgroups for a
//       long one;
//   (c) the combine: a_j += u_{nc+j}, (beta a + alpha b + c) / gamma or / delta, and the zero tails.
// Integer arithmetic only.  This header holds the per-element functions of (a), host + device code
// (tests/native/setup_host_test.cpp), and the entry point; the kernels are in setup_impl.hpp, compiled once per curve in
// setup_<curve>.hip (the engines' translation units only call the entry point).
#pragma once
#include "field.hpp"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace zk {

// ---------------------------------------------------------------- (a) quotient vectors
// Lagrange coefficients (EvaluationDomain::evaluate_all_lagrange_coefficients for tau outside the domain), w the m-th root:
//   u_i = Z(tau) w^i / (m (tau - w^i)),  Z(tau) = tau^m - 1.          k = Z(tau) / m; root = w; first = 1
template <class F>
struct LagrangeTerm {
  F tau, k, root, root_inv;
  ZK_HD F first() const { return F::one(); }
  ZK_HD void at(const F& wi, F& num, F& den) const {
    num = k * wi;
    den = tau - wi;
  }
};
// CircomReduction::h_query_scalars: the odd entries of ifft_N([tau^j / delta]_{j < N - 1} || 0), N = 2m.  Entry 2i + 1 is
// the geometric sum (1 / (delta N)) sum_{j < N - 1} x_i^j with x_i = tau w2^-(2i+1), w2 the N-th root; with x_i^N = tau^N
//   h_i = (1 / (delta N)) (tau^N - x_i) / (x_i (x_i - 1)).            k = 1 / (delta N); root = w2^-2; first = w2^-1
// x_i = 0 needs tau = 0 and x_i = 1 needs tau^N = 1: the caller refuses both.
template <class F>
struct HTerm {
  F tau, tau_n, k, root, root_inv, start;
  ZK_HD F first() const { return start; }
  ZK_HD void at(const F& yi, F& num, F& den) const {
    F x = tau * yi;
    num = k * (tau_n - x);
    den = x * (x - F::one());
  }
};

// One lane's run: out[i] = num_i / den_i for i in [begin, begin + count), count >= 1, every den_i != 0.  The power of the
// root at `begin` comes from one exponentiation and moves by one product per element.  Montgomery's trick over the run:
// the forward pass leaves the prefix products of the denominators in out[] (each lane reads back only what it wrote), one
// inversion of the total, and the backward pass walks the power of the root down again.
template <class F, class Term>
ZK_HD void quotient_run(const Term& t, size_t begin, size_t count, F* out) {
  F y = t.first() * t.root.pow_u64((uint64_t)begin);
  F acc = F::one(), num, den;
  for (size_t i = 0; i < count; i++) {
    out[begin + i] = acc;                       // den_begin * ... * den_{begin+i-1}
    t.at(y, num, den);
    acc = acc * den;
    if (i + 1 < count) y = y * t.root;
  }
  F inv = acc.inverse_safegcd();                // 1 / (den_begin * ... * den_{begin+count-1})
  for (size_t i = count; i-- > 0;) {
    t.at(y, num, den);
    F pre = out[begin + i];
    out[begin + i] = num * (inv * pre);
    inv = inv * den;
    y = y * t.root_inv;
  }
}

#if defined(__HIPCC__)
class IEngine;
struct DevBuf;
// zk_groth16_setup_scalars for the scalar field FrP (engine_setup.inc.hpp has the argument list); wk: working memory
template <class FrP>
int setup_scalars_run(IEngine* e, DevBuf& wk, const void* const mats[9], size_t nvars, size_t nc, size_t ni, int log_m,
                      const void* trapdoor, size_t tail, void* const out[5], hipStream_t st);
#endif

}  // namespace zk
