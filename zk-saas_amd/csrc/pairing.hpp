// The verifier: optimal-ate pairing (BN254, BLS12-381) and the Groth16 verification equation, on the device.
//
// Replaces ark-ec's `Pairing::multi_pairing` / `final_exponentiation` and ark-groth16's `prepare_verifying_key` /
// `verify_proof` (groth16/examples/sha256.rs:389-415).  This header is the host-side interface the C ABI dispatches
// to; the kernels live in pairing_impl.hpp and are compiled once per curve in their own translation units
// (pairing_bn254.hip, pairing_bls381.hip), apart from the prover's objects.
#pragma once
#include "engine.hpp"

// ark_groth16::PreparedVerifyingKey on the device: gamma_abc_g1 with its doubling tables, -gamma_g2, -delta_g2 (affine) and e(alpha, beta);
// for the batch check alpha and beta themselves, the doubling tables of abc[0] and alpha, and the one of Fq12
struct zk_vk {
  int curve = 0, device = 0;
  size_t n_abc = 0;
  void* abc_d = nullptr;          // [n_abc] G1 affine
  void* abc_table_d = nullptr;    // [n_abc - 1][bits of Fr] XYZZ: 2^k abc[i + 1]
  void* neg_gamma_d = nullptr;    // G2 affine
  void* neg_delta_d = nullptr;    // G2 affine
  void* alpha_beta_d = nullptr;   // [12] Fq
  // what zk_groth16_verify_all reads besides (zk_groth16_verify reads none of it)
  void* rlc_base_d = nullptr;     // [3] G1 affine: the identity, abc[0], alpha
  void* rlc_table_d = nullptr;    // [2][bits of Fr] XYZZ: 2^k abc[0], 2^k alpha
  void* beta_d = nullptr;         // G2 affine
  void* one_d = nullptr;          // [12] Fq: the one of Fq12, what the batch's product is compared with
  ~zk_vk() {
    int cur = -1;                   // zk_groth16_vk_free takes no context: the caller's current device is left as it was
    const bool have = hipGetDevice(&cur) == hipSuccess;
    (void)hipSetDevice(device);
    for (void* p : {abc_d, abc_table_d, neg_gamma_d, neg_delta_d, alpha_beta_d, rlc_base_d, rlc_table_d, beta_d, one_d})
      if (p) (void)hipFree(p);
    if (have && cur != device) (void)hipSetDevice(cur);
  }
};

namespace zk {

class IPairing {
 public:
  virtual ~IPairing() {}
  virtual int multi_pairing(IEngine* e, const void* p_d, const void* q_d, size_t k, size_t count, void* gt_out_d,
                            hipStream_t st) = 0;
  virtual int fq12_selftest(IEngine* e, int op, const void* a_d, const void* b_d, size_t len, void* out_d,
                            hipStream_t st) = 0;
  virtual int vk_prepare(IEngine* e, const void* alpha_g1, const void* beta_g2, const void* gamma_g2, const void* delta_g2,
                         const void* gamma_abc_g1, size_t n_abc, zk_vk* vk) = 0;
  virtual int verify(IEngine* e, const zk_vk* vk, const void* proofs, const void* inputs, size_t n_inputs, size_t count,
                     uint8_t* ok, hipStream_t st) = 0;
  virtual int verify_all(IEngine* e, const zk_vk* vk, const void* proofs, const void* inputs, size_t n_inputs, size_t count,
                         const uint8_t* seed, int* all_ok, void* gt_out, hipStream_t st) = 0;
  // subgroup membership and the verifiers that start from wire bytes (subgroup.hpp, subgroup_impl.hpp)
  virtual int points_subgroup_check(IEngine* e, int group, const void* affine_d, size_t len, uint8_t* ok_d, hipStream_t st) = 0;
  virtual int points_decompress_checked(IEngine* e, int group, const void* bytes_d, size_t len, void* out_affine_d, uint8_t* ok_d,
                                        hipStream_t st) = 0;
  virtual int verify_bytes(IEngine* e, const zk_vk* vk, const void* proof_bytes, const void* input_bytes, size_t n_inputs,
                           size_t count, uint8_t* ok, hipStream_t st) = 0;
  virtual int verify_all_bytes(IEngine* e, const zk_vk* vk, const void* proof_bytes, const void* input_bytes, size_t n_inputs,
                               size_t count, const uint8_t* seed, int* all_ok, void* gt_out, hipStream_t st) = 0;
};

IPairing* pairing_bn254();
IPairing* pairing_bls381();

}  // namespace zk
