/* zksaas.h -- C ABI of the MI355X-native zkSaaS hot path (libzksaas_hip.so).
 *
 * The reference (tangle-network/zk-SaaS, pure Rust) has no FFI seam; the seam is the set of generic
 * Rust functions listed below.  Every entry point here cites the reference function it
 * replaces, so that a thin Rust shim can forward the same arguments.
 *
 * Data layout at the boundary = arkworks in-memory representation:
 *   Fr / Fq      : little-endian u64 limbs in MONTGOMERY form, fully reduced
 *                  (4 limbs: BN254 Fr/Fq, BLS12-381 Fr, BLS12-377 Fr; 6 limbs: BLS12-381/377 Fq).
 *   affine point : x || y (Fq2: c0 || c1), (0,0) = identity sentinel.
 *   group value  : Jacobian X || Y || Z, Z = 0 = identity.
 *   share vectors: what one party holds, `Vec<F>` of length m/l; all-party buffers are [n][m/l]
 *                  (party-major, party p's vector contiguous).
 *
 * Pointers whose name ends in _d are DEVICE pointers (hipMalloc / torch tensors); everything else is
 * host memory.  `stream` is a hipStream_t (NULL = default stream).  All functions return a zk_status;
 * zk_last_error() returns the message and, for ZK_ERR_PROTOCOL, the offending party
 * (mpc-net/src/lib.rs:19-24 MpcNetError).  Nothing here falls back to a CPU implementation.
 */
#ifndef ZKSAAS_H
#define ZKSAAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zk_ctx zk_ctx;

enum zk_curve { ZK_BN254 = 0, ZK_BLS12_381 = 1, ZK_BLS12_377 = 2 };
enum zk_group { ZK_G1 = 1, ZK_G2 = 2 };
/* mpc-net/src/lib.rs:19-24 */
enum zk_status { ZK_OK = 0, ZK_ERR_GENERIC = 1, ZK_ERR_PROTOCOL = 2, ZK_ERR_NOT_CONNECTED = 3, ZK_ERR_BAD_INPUT = 4 };

/* ---- context ------------------------------------------------------------------------------------
 * PackedSharingParams::new(l) (secret-sharing/src/pss.rs:39-66): n = 4l parties, t = l, share domain
 * H_n, secret domain g*H_{l+t}, secret2 domain g*H_{2(l+t)}.  `device` is the HIP device ordinal. */
int zk_ctx_create(int curve, int l, int device, zk_ctx** out);
void zk_ctx_destroy(zk_ctx* ctx);
const char* zk_last_error(zk_ctx* ctx, int* party);
int zk_ctx_n(const zk_ctx* ctx);        /* pp.n */
int zk_ctx_l(const zk_ctx* ctx);        /* pp.l */
size_t zk_fr_bytes(const zk_ctx* ctx);  /* 32 */
size_t zk_fq_bytes(const zk_ctx* ctx);  /* 32 or 48 */
const char* zk_version(void);

/* ---- device memory helpers (so that non-torch hosts can drive the library) ---------------------- */
int zk_malloc(zk_ctx* ctx, size_t bytes, void** out_d);
int zk_free(zk_ctx* ctx, void* p_d);
int zk_memcpy_h2d(zk_ctx* ctx, void* dst_d, const void* src, size_t bytes, void* stream);
int zk_memcpy_d2h(zk_ctx* ctx, void* dst, const void* src_d, size_t bytes, void* stream);
int zk_stream_sync(zk_ctx* ctx, void* stream);

/* ---- share randomness ----------------------------------------------------------------------------------------
 * The t random points of every `pack` (pss.rs:90-122; the reference draws them from thread_rng / test_rng:
 * dfft/mod.rs:251, pack.rs:14, deg_red.rs:108) come from a ChaCha20 stream keyed per context from the operating
 * system's generator; every launch that packs gets fresh nonces, so NO `seed` argument below influences them and two
 * calls never share randomness.  zk_ctx_set_option("rng_replay", 1) (a context option only: nothing in the
 * environment can turn it on) switches to the documented replayable generator (DESIGN.md "Randomness": SplitMix64 over
 * (seed, index)) that the parity tests use to compare shares bit for bit with the oracle -- only then do the `seed`
 * arguments matter.  zk_chacha20_block: the block function (RFC 7539 2.3, words 12..15 = counter, nonce), exported
 * for known-answer tests. */
void zk_chacha20_block(const uint32_t key[8], uint64_t counter, uint64_t nonce, uint32_t out[16]);

/* ---- packed secret sharing over Fr (secret-sharing/src/pss.rs) ------------------------------------
 * `order`: 0 = chunk j packs secrets[j*l .. j*l+l-1]  (pack_vec, dist-primitives/src/utils/pack.rs:8-20)
 *          1 = chunk j packs secrets[j], secrets[j+nchunks], ...  (stride packing, dfft/mod.rs:286-299,
 *              groth16/src/qap.rs:103-112)
 * Share randomness: counter-based PRNG documented in DESIGN.md (chunk j uses indices j*t..j*t+t-1 of
 * stream `seed`).  Output shares_d is [n][nchunks]. */
int zk_pss_pack(zk_ctx* ctx, const void* secrets_d, size_t nchunks, int order, uint64_t seed, void* shares_d,
                void* stream);                                                   /* pss.rs:90-122 pack     */
int zk_pss_det_pack(zk_ctx* ctx, const void* secrets_d, size_t nchunks, int order, void* shares_d,
                    void* stream);                                               /* pss.rs:69-87 det_pack  */
/* shares_d is [nparties][nchunks] for the listed parties (ascending ids); secrets_d gets nchunks*l values in
 * order 0.  unpack requires all n parties (pss.rs:125-138); unpack2 falls back to lagrange_unpack when
 * nparties < n (pss.rs:141-221 unpack2 / lagrange_unpack / unpack_missing_shares). */
int zk_pss_unpack(zk_ctx* ctx, const void* shares_d, size_t nchunks, void* secrets_d, void* stream);
int zk_pss_unpack2(zk_ctx* ctx, const void* shares_d, const uint32_t* parties, int nparties, size_t nchunks,
                   void* secrets_d, void* stream);

/* ---- vector helpers ------------------------------------------------------------------------------ */
int zk_bitrev(zk_ctx* ctx, void* x_d, int log2_len, void* stream);  /* dfft/mod.rs:322-335 fft_in_place_rearrange */
int zk_vec_add(zk_ctx* ctx, void* x_d, const void* y_d, size_t len, void* stream);              /* x += y      */
int zk_vec_scale(zk_ctx* ctx, void* x_d, const void* k, size_t len, void* stream);   /* x *= k (k: Montgomery Fr, host);
                                                                    the 1/Z(g) factor of libsnark_h, ext_wit.rs:78-87 */
int zk_vec_mul_sub(zk_ctx* ctx, void* out_d, const void* a_d, const void* b_d, const void* c_d, size_t len,
                   void* stream);                                   /* out = a*b - c, groth16/src/ext_wit.rs:173-177 */

/* ---- d_fft / d_ifft (dist-primitives/src/dfft/mod.rs) --------------------------------------------
 * zk_fft1: fft1_in_place (:178-208) on `batch` share vectors of length m/l each, in place; `inverse`
 *          selects gen = group_gen_inv.  If add_d != NULL it is added element-wise afterwards (the
 *          `share + in_mask` of :254-258 fused into the last pass).
 * zk_fft2_king: the king closure of fft2_with_rearrange (:264-304): unpack_missing_shares per chunk ->
 *          fft2_in_place (:210-237) -> distribute_powers(g) (:278-280) -> (bit-reverse + stride) pack.
 *          in_d is [nparties][m/l], out_d is [n][m/l] and must not alias in_d.  g (Montgomery Fr, host pointer) may be NULL for 1.
 *          scale_size_inv != 0 additionally multiplies by 1/m (d_ifft's :159 folded in).
 * zk_d_fft / zk_d_ifft: :99-175 for all n parties resident on this device: shares_d [n][m/l], masks [n][m/l] each or
 *          NULL for FftMask::zero.  The result is written to out_d [n][m/l] (shares_d is then left as it was);
 *          out_d == NULL or == shares_d returns it in shares_d.  The local stages run out of place into a
 *          working vector and the king step writes the destination, so neither form costs a copy.
 *          RE-ENTRANT ACROSS STREAMS (round 6): the working memory of zk_d_fft / zk_d_ifft / zk_libsnark_h / zk_circom_h /
 *          zk_d_pp / zk_fft_mask_sample / zk_degred_mask_sample (and of the zk_dist_* forms, per channel) belongs to the
 *          `stream` the call is issued on -- calls on one stream are ordered by it and share a set, calls on different
 *          streams never meet (the reference runs three d_ifft at once on three stream ids, groth16/src/ext_wit.rs:127-159;
 *          tests/test_gpu_hardening.py runs two streams against the serial results).  d_pp's zero-denominator word is per
 *          stream as well.  The point kernels (zk_pss_*_points, zk_deg_red_points, zk_groth16_reconstruct) keep
 *          per-context scratch: order them on one stream. */
int zk_fft1(zk_ctx* ctx, void* shares_d, int log2_m, int inverse, size_t batch, const void* add_d, void* stream);
/* Parity-test access to the BASE-field primitives of the group kernels (arkworks' Fq / Fq2 arithmetic, a22; Montgomery Fq
 * elements on the device): op 0: out[i] = a[i] b[i] - c[i] d[i] (the one-reduction form used for Y3 of every XYZZ
 * formula); op 1: out[2i], out[2i+1] = (a[i] + b[i] u)(c[i] + d[i] u), u^2 = -1 (the Fq2 product of the G2 kernels: three
 * unreduced products and two reductions on 8-limb curves); op 2 + k, k < 16: the lazy-residue forms ([0, 2p), field.hpp)
 * the G1 accumulate kernel keeps its running sums in, operand j entered as x + p when bit j of k is set: out[5i .. 5i+4] =
 * a b, a - b, 2a, a b - c d (canonical; all-ones if a result left [0, 2p)) and the raw word
 * (a == c mod p) | (a == 0 mod p) << 1 (out_d holds 5 len elements). */
int zk_fq_selftest(zk_ctx* ctx, int op, const void* a_d, const void* b_d, const void* c_d, const void* d_d, size_t len,
                   void* out_d, void* stream);
int zk_fft2_king(zk_ctx* ctx, const void* in_d, const uint32_t* parties, int nparties, int log2_m, int inverse,
                 const void* g, int scale_size_inv, int rearrange, uint64_t seed, void* out_d,
                 const void* out_mask_d, void* stream);
int zk_d_fft(zk_ctx* ctx, void* shares_d, const void* in_mask_d, const void* out_mask_d, int rearrange,
             int log2_m, uint64_t seed, void* out_d, void* stream);
int zk_d_ifft(zk_ctx* ctx, void* shares_d, const void* in_mask_d, const void* out_mask_d, int rearrange,
              int log2_m, const void* g, uint64_t seed, void* out_d, void* stream);
/* FftMask::sample (:30-85): in_mask_d/out_mask_d are [n][m/l]. */
int zk_fft_mask_sample(zk_ctx* ctx, int rearrange, const void* g, int inverse, int log2_m, uint64_t seed,
                       void* in_mask_d, void* out_mask_d, void* stream);

/* ---- deg_red / d_pp over Fr (dist-primitives/src/utils/deg_red.rs:80-126, dpp/mod.rs:15-87) ------
 * x_d [n][len] in place; masks [n][len] or NULL. */
int zk_deg_red(zk_ctx* ctx, void* x_d, const void* in_mask_d, const void* out_mask_d, size_t len, uint64_t seed,
               void* stream);
/* The same when only `nparties` parties' vectors reached the king (mpc-net/src/ser_net.rs:57-94): x_d is
 * [nparties][len] for the listed ascending ids (masks, if any, in the same order for in_mask and [n][len] for
 * out_mask); the king reconstructs through lagrange_unpack (pss.rs:170-221) and every one of the n parties gets a
 * fresh share in out_d [n][len]. */
int zk_deg_red_parties(zk_ctx* ctx, const void* x_d, const uint32_t* parties, int nparties, const void* in_mask_d,
                       const void* out_mask_d, size_t len, uint64_t seed, void* out_d, void* stream);
int zk_degred_mask_sample(zk_ctx* ctx, size_t len, uint64_t seed, void* in_mask_d, void* out_mask_d,
                          void* stream);                              /* deg_red.rs:40-66 with gen = 1 */
/* num_d, den_d [n][len]; out_d [n][len].  Returns ZK_ERR_GENERIC if a reconstructed denominator is zero
 * (the reference panics on inverse().unwrap(), dpp/mod.rs:55). */
int zk_d_pp(zk_ctx* ctx, const void* num_d, const void* den_d, const void* in_mask_d, const void* out_mask_d,
            size_t len, uint64_t seed, void* out_d, void* stream);

/* deg_red over GROUP elements (deg_red.rs:80-126 with T = G; DegRedMask::sample with a group generator, :40-66):
 * x_d, masks, out_d are [n][len] affine points (out_d must not alias x_d); gen_affine (host) = the generator whose
 * random multiples serve as the t fresh random points of the king's re-pack and as mask values. */
int zk_deg_red_points(zk_ctx* ctx, int group, const void* x_d, const void* in_mask_d, const void* out_mask_d, size_t len,
                      const void* gen_affine, uint64_t seed, void* out_d, void* stream);
int zk_degred_mask_sample_points(zk_ctx* ctx, int group, const void* gen_affine, size_t len, uint64_t seed,
                                 void* in_mask_d, void* out_mask_d, void* stream);

/* ---- MSM / d_msm (dist-primitives/src/dmsm/mod.rs) ---------------------------------------------------
 * zk_msm: G::msm(bases, scalars) (:73, ark-ec VariableBaseMSM): bases affine, scalars Montgomery Fr;
 *         out (HOST pointer) receives one Jacobian point.  `len_bases != len_scalars` -> ZK_ERR_GENERIC
 *         carrying min(len) like arkworks' Err(usize).
 * zk_d_msm: :59-102 for all n parties on this device: bases_d [n][len], scalars_d [n][len];
 *         in_mask/out_mask: n Jacobian points each (host) or NULL for MsmMask::zero; out: n Jacobian points. */
int zk_msm(zk_ctx* ctx, int group, const void* bases_d, size_t len_bases, const void* scalars_d,
           size_t len_scalars, void* out, void* stream);
int zk_d_msm(zk_ctx* ctx, int group, const void* bases_d, const void* scalars_d, size_t len, const void* in_mask,
             const void* out_mask, void* out, void* stream);

/* ---- dealer: fixed-base multiplication -----------------------------------------------------------------
 * out_affine_d[i] = scalars_d[i] * Base for one affine base point (host pointer).  With the trapdoor this is how
 * CRS elements are produced, and -- because det_pack is linear -- how PackedProvingKeyShare::
 * pack_from_arkworks_proving_key (groth16/src/proving_key.rs:47-123) is evaluated: det_pack the discrete logs
 * with zk_pss_det_pack, then multiply the base. */
/* pack / det_pack over GROUP elements (pss.rs:69-122 with T = curve point): points_d is [nchunks][points_per_chunk]
 * affine with points_per_chunk = l (det_pack: PackedProvingKeyShare::pack_from_arkworks_proving_key,
 * proving_key.rs:72-86) or l + t (pack with caller-supplied random points: MsmMask::sample, dmsm/mod.rs:34-38);
 * shares_d is [n][nchunks] affine.  No trapdoor is needed (compare zk_base_mul). */
int zk_pss_pack_points(zk_ctx* ctx, int group, const void* points_d, size_t nchunks, int points_per_chunk,
                       void* shares_d, void* stream);
int zk_base_mul(zk_ctx* ctx, int group, const void* base_affine, const void* scalars_d, size_t len,
                void* out_affine_d, void* stream);
/* zk_base_mul_few: the same product for a FEW scalars (the share scalars of MsmMask::sample, dmsm/mod.rs:34-38: 2 n per
 * mask): a group of 8 lanes per scalar over the base's 8-bit window table, folded in a tree -- zk_base_mul gives a lane a
 * whole scalar, which is right at 2^17 scalars and a serial chain at 64.  scalars_d: Montgomery Fr (device), base_affine:
 * host; out_jacobian_d: len JACOBIAN points (device; no inversion; a zero scalar gives Z = 0).  len above 4096 returns
 * ZK_ERR_BAD_INPUT: use zk_base_mul. */
int zk_base_mul_few(zk_ctx* ctx, int group, const void* base_affine, const void* scalars_d, size_t len,
                    void* out_jacobian_d, void* stream);

/* ---- Groth16 composition (groth16/src/ext_wit.rs, prove.rs, examples/sha256.rs:32-129) -------------------
 * All n parties' shares live on this device.  Mask slots may be NULL (the *::zero() masks).
 * fft masks 0..2: the three d_ifft (a, b, c), 3..5: the three d_fft (ext_wit.rs:127-170), each [n][m/l];
 * degred: [n][m/l]; msm masks in the order A (S), B-in-G1 (H), B-in-G2 (V), C.w (W), C.u (U): n Jacobian
 * points each, host memory (sha256.rs:226-291). */
typedef struct zk_groth16_masks {
  const void* fft_in[6];
  const void* fft_out[6];
  const void* degred_in;
  const void* degred_out;
  const void* msm_in[5];
  const void* msm_out[5];
} zk_groth16_masks;

/* PackedProvingKeyShare for all parties (groth16/src/proving_key.rs:18-37): share vectors are device
 * buffers [n][len] of affine points, the single elements are host affine points. */
typedef struct zk_crs_share {
  const void* s_d;   /* a_query[1..]      G1 [n][len_a] */
  const void* h_d;   /* b_g1_query[1..]   G1 [n][len_a] */
  const void* v_d;   /* b_g2_query[1..]   G2 [n][len_a] */
  const void* w_d;   /* l_query           G1 [n][len_w] */
  const void* u_d;   /* h_query           G1 [n][len_u], len_u = m/l */
  size_t len_a, len_w, len_u;
  const void *a_query0, *b_g1_query0, *delta_g1, *alpha_g1, *beta_g1; /* G1 */
  const void *b_g2_query0, *delta_g2, *beta_g2;                       /* G2 */
} zk_crs_share;

/* circom_h (ext_wit.rs:104-181): qap_*_d [n][m/l] are not modified; h_d [n][m/l]. */
int zk_circom_h(zk_ctx* ctx, const void* qap_a_d, const void* qap_b_d, const void* qap_c_d, int log2_m,
                const zk_groth16_masks* masks, uint64_t seed, void* h_d, void* stream);
/* dsha256 (sha256.rs:32-129) for all parties: a_share_d [n][len_a] = shares of assignment[1..], ax_share_d
 * [n][len_w] = shares of the aux assignment; r, s: Montgomery Fr (host) -- every party holds r and s in the
 * clear.  pi_a / pi_c: n Jacobian G1 points, pi_b: n Jacobian G2 points (host). */
int zk_groth16_prove(zk_ctx* ctx, const zk_crs_share* crs, const void* qap_a_d, const void* qap_b_d,
                     const void* qap_c_d, const void* a_share_d, const void* ax_share_d, const void* r, const void* s,
                     int log2_m, const zk_groth16_masks* masks, uint64_t seed, void* pi_a, void* pi_b, void* pi_c,
                     void* stream);

/* ---- multi-GPU building blocks (the n parties spread over several ranks, king = rank 0) ------------------
 * zk_d_msm_local: this rank's share of d_msm's king step (dmsm/mod.rs:85-86): sum over its `nparties` parties
 *   (ids first_party ..) of coef_p * (G::msm(bases_p, scalars_p) + in_mask_p), coef_p = sum_k unpack2 row k.
 *   bases_d / scalars_d are [nparties][len]; in_mask: nparties Jacobian points (host) or NULL; out: one
 *   Jacobian point (host).  Summing the ranks' outputs (zk_group_add) gives the king's broadcast value.
 * zk_groth16_assemble: prove.rs:40-56, 99-110, 148-158, 229-235 from the five summed d_msm values
 *   sums[0..4] = S, H, V (G2), W, U (Jacobian, host). */
int zk_d_msm_local(zk_ctx* ctx, int group, const void* bases_d, const void* scalars_d, size_t len, int first_party,
                   int nparties, const void* in_mask, void* out, void* stream);
int zk_group_add(zk_ctx* ctx, int group, const void* a, const void* b, void* out);
/* Introspection (no reference counterpart; ark-ec picks its window inside VariableBaseMSM::msm): the Pippenger plan
 * zk_msm uses for `len` points of `group`: plan[0] = widest window in bits, plan[1] = number of windows,
 * plan[2] = points per accumulate lane, plan[3] = base-field multiplications per mixed addition (10 for G1,
 * 28 for G2 over Fq2).  Benchmarks use it to turn a launch duration into multiplications per second. */
int zk_msm_plan(zk_ctx* ctx, int group, size_t len, int plan[4]);
/* Fixed-base tables (no reference counterpart; arkworks has FixedBase::msm for setup only).  A prover service proves
 * many witnesses against one CRS: zk_msm_precompute builds, for the affine vector bases_d [len] (e.g. one query of
 * zk_crs_share, all parties: len = n * len_a), the multiples 2^(16 j) * P_i, j < 16, owned by the context (16 x the
 * size of the vector).  Every later zk_msm / zk_d_msm / zk_groth16_prove whose base pointer lies inside a registered
 * vector uses its table: all windows then share one bucket set (one bucket reduction, no doublings in the final
 * fold, 16 instead of 20-22 mixed additions per point).  Results are the same group elements.
 * zk_free drops the tables of vectors inside the freed allocation; for memory the caller frees itself (e.g. a torch
 * tensor) call zk_msm_forget first -- tables are found by address.
 * zk_msm_forget drops the table of bases_d (returns ZK_ERR_BAD_INPUT if there is none); zk_msm_table_info writes
 * info[0] = window bits, info[1] = digit windows of the table that covers bases_d (zeros if none). */
int zk_msm_precompute(zk_ctx* ctx, int group, const void* bases_d, size_t len, void* stream);
int zk_msm_forget(zk_ctx* ctx, const void* bases_d);
int zk_msm_table_info(zk_ctx* ctx, int group, const void* bases_d, int info[2]);
/* Tunables of this context (no reference counterpart).  "rng_replay": see "share randomness".  "msm_bigsort_min": point count from which zk_msm sorts with
 * the two-level LDS counting sort instead of global atomics (default 16384 = 2^14; tests force both paths with it).
 * "msm_table_c": window bits (8..22, 0 = default; "msm_table_c_g2" sets G2 alone) of tables built by later zk_msm_precompute calls.
 *   Default: by the vector's length -- G1 15 bits up to 2^17 points, 16 below 2^19, 17 below 2^22, 20 from there; G2 15 below 2^20, 19 from
 *   there (a table folds all windows into one bucket set: too few buckets for a long vector sends every bucket through the
 *   heavy-bucket path; csrc/msm.hpp table_c_auto).
 * "king_alltoall": 1 = the zk_dist_* king rounds of d_fft / d_ifft / deg_red (and everything composed of them) run as
 * all-to-all: every present rank is king of a contiguous chunk range (zk_net_alltoall twice per round) instead of
 * gather -> rank 0 -> scatter; identical results; every rank of a net must choose alike (default 0).
 * "msm_c" / "msm_c_g2": window bits (2..20, 0 = the cost model) of table-free MSMs (tests force widths with it).
 * "h_first_log_m": domains of 2^value and up run circom_h and every MSM's sort ahead of the accumulate kernels (default 20).
 * "host_threads": workers of the context's host pool (0 = by the core count, else >= 4; before the first proof).
 * "wait_deadline_ms": bound of every host-side wait inside the prover and MSM entry points (an MSM chain's completion event,
 *   a gate between two launching threads, a pool task; default 120000, 0 = unbounded): zk_groth16_prove / _wait / _batch_wait,
 *   zk_groth16_msms_finish, the zk_dist_*groth16* calls, zk_msm, zk_msm_batch, zk_d_msm, zk_d_msm_parties, zk_d_msm_local and
 *   zk_dist_d_msm.  On expiry the call returns ZK_ERR_GENERIC naming what it waited for (a prover job's gates and events go
 *   to stderr), the MSM workspace it used is never reused and the context is wedged: every later prover and MSM call fails
 *   at once ("wedged": destroy the context).  So none of them can block for ever (the net's own rounds have
 *   zk_net_set_timeout_ms).
 * "dist_deadline": 1 = the zk_dist_* calls return only with their data-plane work done (zk_net_sync inside).
 * "pack_glv": 0 = zk_pss_pack_points at two points per chunk walks the parties' full-length scalars; 1 (default) = the
 *   scalars are split by the curve's endomorphism phi(x, y) = (beta x, y) = lambda (x, y) into two half-length parts (half
 *   the doubling chain; the same points).  Before the first zk_pss_pack_points of the context.
 * Nothing is read from the environment.  Unknown name or value out of range -> ZK_ERR_BAD_INPUT. */
int zk_ctx_set_option(zk_ctx* ctx, const char* name, long long value);
/* Memory-model note (csrc/msm.hpp msm_hist): the last workgroup of a sort's histogram finds out that it is the last through a
 * RELAXED device-scope ticket (an acquire fence follows in that workgroup; the release side would write back an XCD's L2 per
 * workgroup: -3.8 % of a SHA-256 proof, measured).  Correctness rests on gfx950 behaviour, not on the HIP memory model: the
 * counts are device-scope atomic read-modify-writes performed at the memory side, every wave holds the return values of its
 * adds before the barrier that precedes the ticket, and the scanning workgroup reads them with device-scope atomic loads.
 * -DZK_HIST_TICKET_ACQ_REL=1 builds the formally ordered form; tests/test_gpu_msm.py::test_concurrent_sorts_stress runs
 * hundreds of concurrent sorts against serial results on the shipped build. */
/* MsmMask::sample (dmsm/mod.rs:21-47): l random scalars x_i (stream `seed`), mask values x_i * gen, out value
 * -(sum), both packed with t random group elements each (streams seed^0x1111, seed^0x2222; a random group element
 * is a random multiple of gen).  gen_affine: the group generator (host, affine Montgomery); in_mask / out_mask
 * (HOST) receive n Jacobian points each. */
int zk_msm_mask_sample(zk_ctx* ctx, int group, const void* gen_affine, uint64_t seed, void* in_mask, void* out_mask);
/* zk_groth16_deal_masks: ALL preprocessing material of nproofs proofs in one call (groth16/examples/sha256.rs:226-291:
 * six FftMask::sample, one DegRedMask::sample, five MsmMask::sample per proof).  masks[b] names the DESTINATIONS, of
 * exactly the kinds zk_groth16_prove reads (fft_in/out[k], degred_in/out: device [n][m/l] Fr; msm_in/out[k]: host, n
 * Jacobian points, k = 2 in G2), so the filled structs go to zk_groth16_prove / _async / _batch as they are.  A slot
 * whose two pointers are NULL is skipped (it stays the ::zero() mask); one NULL pointer of a pair, a G2 slot without
 * g2_gen_affine or on a curve without G2 -> ZK_ERR_BAD_INPUT.  FFT masks k < 3 are FftMask::sample with rearrange, g =
 * the 2m-th root of unity and the inverse transform (the three d_ifft of ext_wit.rs:127-142), k >= 3 the plain forward
 * form; the DegRedMask is over m/l chunks; the MsmMasks are multiples of the generators (scalar form of
 * zk_msm_mask_sample), computed on the device: one launch for all share scalars, one zk_base_mul_few launch per group.
 * Replay mode: proof b draws what the single samplers draw with seed + 16 b (the stride of zk_groth16_prove_batch) + k
 * for FFT mask k, + 6 for deg_red, + 7 + k for MSM mask k; otherwise fresh nonces, none used twice.  Any nproofs >= 1
 * (16 proofs per internal pass).  Returns with the host points written and the device masks ordered on `stream`. */
int zk_groth16_deal_masks(zk_ctx* ctx, int nproofs, int log2_m, const void* g1_gen_affine, const void* g2_gen_affine,
                          uint64_t seed, const zk_groth16_masks* masks, void* stream);

/* ---- circom front end (what the reference takes from ark-circom + groth16/src/qap.rs) ------------------
 * zk_r1cs_qap: qap.rs:42-89 (`qap::<F, D>()` for the circom reduction): A and B as CSR on the device
 *   (row_ptr [num_constraints+1] u32, col u32 wire indices, val Montgomery Fr), w_d the full assignment
 *   [num_variables]; writes a, b, c [2^log_m] in natural order: a_i = <A_i,w>, b_i = <B_i,w>, c_i = a_i*b_i,
 *   a[nc .. nc+ni) = w[0 .. ni), zero padding.  2^log_m < nc + ni -> ZK_ERR_BAD_INPUT; a wire index
 *   >= num_variables -> ZK_ERR_GENERIC.
 * zk_fr_to_bytes / zk_fr_from_bytes: ark-serialize CanonicalSerialize / CanonicalDeserialize of Fr elements
 *   (little-endian canonical integers, the payload of mpc-net frames, ser_net.rs:24-25) for device vectors;
 *   from_bytes returns ZK_ERR_GENERIC when an element is >= the modulus (arkworks: InvalidData). */
int zk_r1cs_qap(zk_ctx* ctx, const void* a_row_ptr_d, const void* a_col_d, const void* a_val_d,
                const void* b_row_ptr_d, const void* b_col_d, const void* b_val_d, const void* w_d,
                size_t num_variables, size_t num_constraints, size_t num_instance, int log_m, void* a_out_d,
                void* b_out_d, void* c_out_d, void* stream);
/* zk_groth16_deal_witness: a device-resident assignment w_d -> the five share vectors zk_groth16_prove takes (QAP::pss,
 * groth16/src/qap.rs:91-135, and the two pack_from_witness of sha256.rs:131-156, 205-224) without a trip through the
 * host: zk_r1cs_qap (same CSR arguments), bit reversal and pack at order 1 with seeds seed + 0, 1, 2 -> qap_a/b/c_d
 * [n][m/l]; w[1..] packed with seed + 3 -> a_share_d [n][len_a], w[ni..] with seed + 4 -> ax_share_d [n][len_w], both
 * straight from w_d with the last chunk's tail read as zero.  len_a = ceil((nv - 1) / l) and len_w = ceil((nv - ni) / l)
 * are written to *len_a / *len_w (either may be NULL); with all five outputs NULL that is all the call does (size query). */
int zk_groth16_deal_witness(zk_ctx* ctx, const void* a_row_ptr_d, const void* a_col_d, const void* a_val_d,
                            const void* b_row_ptr_d, const void* b_col_d, const void* b_val_d, const void* w_d,
                            size_t num_variables, size_t num_constraints, size_t num_instance, int log_m, uint64_t seed,
                            void* qap_a_d, void* qap_b_d, void* qap_c_d, void* a_share_d, void* ax_share_d, size_t* len_a,
                            size_t* len_w, void* stream);
/* zk_groth16_setup_scalars: the circuit-specific setup in the exponent (ark_groth16::generate_parameters with the circom
 * reduction, what groth16/examples/sha256.rs calls circuit_specific_setup, before its fixed-base multiplications): R1CS
 * and trapdoor -> the discrete logs of the five CRS vectors, LibsnarkReduction::instance_map_with_evaluation +
 * CircomReduction::h_query_scalars, on the device.  A, B and C as CSR exactly as zk_r1cs_qap takes them (row_ptr u32
 * [num_constraints + 1], col u32 wire indices, val Montgomery Fr; a matrix without nonzeros may pass NULL col / val).
 * trapdoor (HOST): alpha, beta, gamma, delta, tau, five Montgomery Fr.  With u_i the Lagrange coefficients of the size-m
 * domain (m = 2^log_m) at tau, outputs are Montgomery Fr device vectors in natural order:
 *   a_query_d   [nv]      a_j = sum_i u_i A[i][j], plus u_{nc + j} for j < ni
 *   b_query_d   [nv]      b_j = sum_i u_i B[i][j]
 *   gamma_abc_d [ni]      (beta a_j + alpha b_j + c_j) / gamma for j < ni       (c_j = sum_i u_i C[i][j])
 *   l_query_d   [nv - ni] (beta a_j + alpha b_j + c_j) / delta for j >= ni
 *   h_query_d   [m]       the odd entries of ifft_2m([tau^j / delta]_{j < 2m - 1} || 0)
 * `tail_zeros` zero elements are written behind each of a_query, b_query, l_query and h_query (so that l-chunked views
 * handed to zk_pss_det_pack read zeros past the end); gamma_abc has no tail.  Any output pointer may be NULL: that vector
 * is not written.  Ordered on `stream`; the call returns after the kernels that validate the wire indices have run.
 * Errors: 2^log_m < nc + ni, ni == 0, ni > nv or a 2m domain beyond the field's two-adicity -> ZK_ERR_BAD_INPUT; a wire
 * index >= nv -> ZK_ERR_GENERIC (as zk_r1cs_qap); a degenerate trapdoor -> ZK_ERR_BAD_INPUT naming the element: gamma = 0,
 * delta = 0, tau = 0 or tau^(2m) = 1 (tau inside the size-2m domain), checked on the host before any launch.  arkworks
 * would return an indicator vector for tau in the domain; no honest setup keeps such a tau, and refusing it keeps every
 * denominator of the call nonzero.  The context stays usable after every error.  Device engine only. */
int zk_groth16_setup_scalars(zk_ctx* ctx, const void* a_row_ptr_d, const void* a_col_d, const void* a_val_d,
                             const void* b_row_ptr_d, const void* b_col_d, const void* b_val_d, const void* c_row_ptr_d,
                             const void* c_col_d, const void* c_val_d, size_t num_variables, size_t num_constraints,
                             size_t num_instance, int log_m, const void* trapdoor, size_t tail_zeros, void* a_query_d,
                             void* b_query_d, void* l_query_d, void* h_query_d, void* gamma_abc_d, void* stream);
/* zk_pss_unpack_robust: the error-correcting unpack.  The n = 4l shares of a chunk are a Reed-Solomon word over the share
 * domain H_n; for a polynomial of degree < `dimension` (2l for packed shares, 4l - 1 for their products) the word has
 * redundancy that zk_pss_unpack / zk_pss_unpack2 do not use.  secret-sharing/src/gao.rs:47-84 decode_to_message per chunk, with the early return and the failure checks
 * its todo lines ask for.  A verdict per chunk: the call returns ZK_OK whatever the shares are.
 * With cap = (n - dimension) / 2:
 *   status 0  clean: the interpolant of the n shares has degree < dimension; it is the message h
 *   status 1  corrected: a polynomial h of degree < dimension (it is unique) differs from the shares in 1 .. cap positions;
 *             bit p of errpos is set exactly for those parties
 *   status 2  failed: no such polynomial; message and secrets are written as zeros, errpos as 0
 * For status 0 and 1 the secrets are h(g w_2l^i), i < l: zk_pss_unpack's result on a clean word of degree < 2l,
 * zk_pss_unpack2's on a clean product word.  More than cap wrong shares either fail or -- with probability about
 * n^cap / r -- land within cap of another codeword, which is a legitimate status 1.
 * Only all n parties: shares_d is [n][nchunks] in party order.  With parties absent -- a dropout, or a party left out
 * because it is known to lie -- the call is zk_pss_unpack_robust_parties below.
 * Errors: dimension outside 1 .. n - 1, or NULL shares_d / status_d with nchunks > 0 -> ZK_ERR_BAD_INPUT (the context stays
 * usable); nchunks == 0 is ZK_OK.  No host synchronisation inside the call: everything is ordered on `stream`, working
 * memory comes from the stream's workspace as in zk_groth16_setup_scalars.  Device engine only. */
int zk_pss_unpack_robust(zk_ctx* ctx, const void* shares_d /* [n][nchunks] */, size_t nchunks, int dimension,
                         void* secrets_d   /* [nchunks*l], order 0, or NULL */,
                         void* message_d   /* [dimension][nchunks] coefficients of h, or NULL */,
                         uint8_t* status_d /* [nchunks] */,
                         uint32_t* errpos_d /* [nchunks], or NULL */,
                         uint64_t* summary_d /* [3 + n]: clean, corrected, failed, then per party the number of
                                                chunks in which its share was corrected; or NULL */,
                         void* stream);
/* zk_pss_unpack_robust_parties: the error-correcting unpack of the shares of a party list S: dropouts (erasures) and wrong
 * shares (errors) in one chunk.  secret-sharing/src/gao.rs:11-84 over the points of S, with the party list of
 * unpack_missing_shares / lagrange_unpack, secret-sharing/src/pss.rs:141-221.  shares_d is [nparties][nchunks], row i the
 * shares of party parties[i]; parties (HOST) holds ascending ids below n, NULL stands for 0 .. nparties - 1.
 * With k = dimension and cap = (nparties - k) / 2, rounded down:
 *   status 0  the interpolant through the shares on { w_n^p : p in S } has degree < k; it is the message h
 *   status 1  a polynomial h of degree < k (it is unique) differs from the listed shares in 1 .. cap places; bit p of
 *             errpos is set exactly for those parties -- p is the party's id, not its place in the list -- and never
 *             for an absent party
 *   status 2  neither; message and secrets are written as zeros, errpos as 0
 * secrets_d, message_d [dimension][nchunks], status_d, errpos_d and summary_d [3 + n] (per party id) are
 * zk_pss_unpack_robust's, and with nparties == n every output equals that call's.  A party named in errpos once can be
 * left out of the list afterwards: its chunks are clean again, at the cost of the clean path.
 * Errors: a list that is not strictly ascending or holds an id >= n, nparties outside 1 .. n, dimension outside
 * 1 .. n - 1, or NULL shares_d / status_d with nchunks > 0 -> ZK_ERR_BAD_INPUT; nparties <= dimension ->
 * ZK_ERR_PROTOCOL (too few shares, as zk_pss_unpack2, pss.rs:183-186); the context stays usable.  nchunks == 0 is ZK_OK.
 * No host synchronisation, working memory from the stream's workspace.  Device engine only. */
int zk_pss_unpack_robust_parties(zk_ctx* ctx, const void* shares_d /* [nparties][nchunks] */,
                                 const uint32_t* parties /* host, ascending ids, NULL = 0..nparties-1 */, int nparties,
                                 size_t nchunks, int dimension, void* secrets_d, void* message_d, uint8_t* status_d,
                                 uint32_t* errpos_d, uint64_t* summary_d, void* stream);
/* zk_pss_repair: the verdicts of zk_pss_unpack_robust, written back into the shares -- a corrected SHARE MATRIX, which the
 * king steps below (and any other consumer of shares) then read unchanged.  secret-sharing/src/gao.rs:47-84 per chunk, as
 * zk_pss_unpack_robust; the value written is the re-encoding of the decoded message, h(w_n^p).
 * status_d, errpos_d and summary_d are exactly zk_pss_unpack_robust's on the same input, with the same encoding and the same
 * error returns; summary_d is overwritten by the call.  shares_d changes only as follows: in a status-1 chunk the element of
 * every party named in errpos is overwritten with h(w_n^p).  Every other element keeps its bytes: clean chunks, failed
 * chunks, and the right shares of a corrected chunk.  A second call on the result reports the former status-1 chunks clean.
 * All n parties only.  No host synchronisation, working memory from the stream's workspace.  Device engine only. */
int zk_pss_repair(zk_ctx* ctx, void* shares_d /* [n][nchunks], in place */, size_t nchunks, int dimension,
                  uint8_t* status_d /* [nchunks] */, uint32_t* errpos_d /* [nchunks], or NULL */,
                  uint64_t* summary_d /* [3 + n], or NULL */, void* stream);
/* Checked king rounds: each takes the unchecked call's arguments followed by status_d [chunks], errpos_d (or NULL) and
 * summary_d [3 + n] (or NULL), runs zk_pss_repair on the word the king receives and then the unchecked king on the repaired
 * matrix.  On honest input the output is bit for bit the unchecked call's under the same seed; on a repaired word it is the
 * honest output.  A failed chunk (status 2) is NOT an error return: its shares go to the king as received, and the caller
 * reads summary_d[2].  All n parties on this device; the unchecked calls are unchanged.  Device engine only.
 *
 * zk_fft2_king_checked: the king of d_fft / d_ifft (dist-primitives/src/dfft/mod.rs:264-304) on in_d [n][m/l], which is
 * repaired IN PLACE at dimension 2l (gao.rs: up to l wrong shares per chunk are corrected).  status_d is [m/l], indexed by
 * input chunk, which is column k of in_d.  nparties != n -> ZK_ERR_BAD_INPUT: the party list is the unchecked call's.
 * in_d == out_d -> ZK_ERR_BAD_INPUT as for zk_fft2_king: the king's workgroups exchange chunks, it never runs in place. */
int zk_fft2_king_checked(zk_ctx* ctx, void* in_d, const uint32_t* parties, int nparties, int log2_m, int inverse,
                         const void* g, int scale_size_inv, int rearrange, uint64_t seed, void* out_d,
                         const void* out_mask_d, uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d, void* stream);
/* zk_d_fft_checked / zk_d_ifft_checked: zk_d_fft / zk_d_ifft with the king's word checked.  The word is what the
 * reference's king receives, fft1(x) + in_mask, for d_ifft fft1(x) / m + in_mask (dfft/mod.rs:159, :254-258, the king
 * :264-304); dimension 2l, so a party whose whole vector is wrong -- and up to l of them -- is named and corrected.
 * shares_d is left untouched when out_d is given, as in the unchecked calls; status_d is [m/l]. */
int zk_d_fft_checked(zk_ctx* ctx, void* shares_d, const void* in_mask_d, const void* out_mask_d, int rearrange, int log2_m,
                     uint64_t seed, void* out_d, uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d, void* stream);
int zk_d_ifft_checked(zk_ctx* ctx, void* shares_d, const void* in_mask_d, const void* out_mask_d, int rearrange, int log2_m,
                      const void* g, uint64_t seed, void* out_d, uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d,
                      void* stream);
/* zk_deg_red_checked: zk_deg_red with the king's word x + in_mask checked (dist-primitives/src/utils/deg_red.rs:99-115).
 * The word has degree up to 4l - 2, so the dimension is 4l - 1 and cap = (n - 4l + 1) / 2 = 0 (gao.rs): this is DETECTION
 * ONLY.  A chunk's status is 0 or 2, errpos is always 0, and nothing is ever rewritten: the output equals zk_deg_red's on the
 * same input.  status_d is [len]. */
int zk_deg_red_checked(zk_ctx* ctx, void* x_d, const void* in_mask_d, const void* out_mask_d, size_t len, uint64_t seed,
                       uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d, void* stream);
/* zk_pss_repair_parties: zk_pss_repair for the shares of a party list S -- the verdicts of zk_pss_unpack_robust_parties,
 * written back into the shares.  secret-sharing/src/gao.rs:11-84 over the points of S, the party list of
 * unpack_missing_shares, secret-sharing/src/pss.rs:141-221.  shares_d is [nparties][nchunks], row i the shares of party
 * parties[i]; parties (HOST) holds ascending ids below n, NULL stands for 0 .. nparties - 1.
 * status_d, errpos_d (by party id), summary_d [3 + n] and every error return are exactly zk_pss_unpack_robust_parties' on
 * the same input: ZK_ERR_PROTOCOL for nparties <= dimension included, and a status 1 that names an absent party is status 2.
 * WRITTEN: in a status-1 chunk, the element in row i of every listed party parties[i] named in the final errpos becomes
 * h(w_n^parties[i]).  NOT WRITTEN: clean chunks, failed chunks, the right shares of a corrected chunk; an absent party has
 * no row, and its share is not recovered.  A second call on the result reports the former status-1 chunks clean.  With
 * nparties == n the outputs and the bytes written are zk_pss_repair's.  A party named in errpos once can be left out of the
 * list afterwards: its chunks are clean again and none reaches the decoder.
 * No host synchronisation, working memory from the stream's workspace.  Device engine only. */
int zk_pss_repair_parties(zk_ctx* ctx, void* shares_d /* [nparties][nchunks], in place */,
                          const uint32_t* parties /* host, ascending ids, NULL = 0..nparties-1 */, int nparties,
                          size_t nchunks, int dimension, uint8_t* status_d /* [nchunks] */,
                          uint32_t* errpos_d /* [nchunks], or NULL */, uint64_t* summary_d /* [3 + n], or NULL */,
                          void* stream);
/* zk_pss_repair_range: parity access to the RANGE form of zk_pss_repair_parties, which the checked rounds on the net run
 * where every rank is king of a range of chunks (zk_dist_*_checked with the option king_alltoall; like zk_fq_selftest, for
 * tests).  The word of len chunks is not contiguous: shares_d is a block [nparties][stride] of which columns 0 .. cnt - 1
 * are valid, and column c is chunk (base + c + len - shift) mod len of the word -- the layout in which the king of a range
 * receives it (dist-primitives/src/dfft/mod.rs:264-304 reads the whole word; here a rank holds its range).  Shares are read
 * and rewritten at row * stride + c for c < cnt only: columns cnt .. stride - 1 are neither read nor written.  status_d and
 * errpos_d are [len] and written at the mapped chunks only; summary_d counts the cnt chunks (cnt == 0: all zeros).
 * With stride == cnt == len, base == 0 and shift == 0 every output and every byte written is zk_pss_repair_parties'.
 * Errors: those of zk_pss_repair_parties; cnt > stride, cnt > len, base >= len or shift > len is ZK_ERR_BAD_INPUT. */
int zk_pss_repair_range(zk_ctx* ctx, void* shares_d /* [nparties][stride], in place */,
                        const uint32_t* parties /* host, ascending ids, NULL = 0..nparties-1 */, int nparties, size_t stride,
                        uint32_t cnt, uint32_t len, uint32_t base, uint32_t shift, int dimension,
                        uint8_t* status_d /* [len] */, uint32_t* errpos_d /* [len], or NULL */,
                        uint64_t* summary_d /* [3 + n], or NULL */, void* stream);
/* Checked king rounds with a party list: the calls above for the case that only the listed parties' shares reached the king
 * (dist-primitives/src/dfft/mod.rs:264-304 with the list of unpack_missing_shares, pss.rs:141-221) -- a dropout, or a party
 * left out because an earlier report named it.  Each runs zk_pss_repair_parties at dimension 2l on the word the king
 * receives and then the unchecked king with the same list.  The refusals are zk_pss_repair_parties': a bad list is
 * ZK_ERR_BAD_INPUT, nparties <= 2l is ZK_ERR_PROTOCOL -- and the unchecked king's, whose unpack_missing_shares takes a list
 * only with more than 4l - 2 shares (pss.rs:183-186): nparties < 4l - 1 is ZK_ERR_PROTOCOL as it is for zk_fft2_king, so
 * a list is all n parties or n - 1 of them.  Every refusal is made before anything is written.
 * cap = (nparties - 2l) / 2 wrong shares per chunk are corrected and
 * named by party id; a failed chunk is not an error return.  With nparties == n the outputs are the all-parties checked
 * call's.  deg_red has no such form: at dimension 4l - 1 a list of n - 1 parties has no redundancy left, nothing could even
 * be detected.
 *
 * zk_fft2_king_checked_parties: in_d is [nparties][m/l], row i the shares of parties[i], REPAIRED IN PLACE; out_d is
 * [n][m/l].  in_d == out_d -> ZK_ERR_BAD_INPUT.  status_d is [m/l]. */
int zk_fft2_king_checked_parties(zk_ctx* ctx, void* in_d, const uint32_t* parties, int nparties, int log2_m, int inverse,
                                 const void* g, int scale_size_inv, int rearrange, uint64_t seed, void* out_d,
                                 const void* out_mask_d, uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d,
                                 void* stream);
/* zk_d_fft_checked_parties / zk_d_ifft_checked_parties: zk_d_fft_checked / zk_d_ifft_checked when only the listed parties'
 * words reach the king (dfft/mod.rs:159, :254-258, the king :264-304).  shares_d, in_mask_d and the outputs are [n][m/l] as
 * before; only the rows of the listed parties are read: fft1 of row parties[i], (for the inverse: times 1 / m,) plus the
 * in-mask row of parties[i] is row i of the king's word, which is repaired and handed to the king with the list.  The rows
 * of absent parties in shares_d and in_mask_d are never read; shares_d is left untouched when out_d is given.  status_d is
 * [m/l]. */
int zk_d_fft_checked_parties(zk_ctx* ctx, void* shares_d, const uint32_t* parties, int nparties, const void* in_mask_d,
                             const void* out_mask_d, int rearrange, int log2_m, uint64_t seed, void* out_d,
                             uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d, void* stream);
int zk_d_ifft_checked_parties(zk_ctx* ctx, void* shares_d, const uint32_t* parties, int nparties, const void* in_mask_d,
                              const void* out_mask_d, int rearrange, int log2_m, const void* g, uint64_t seed, void* out_d,
                              uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d, void* stream);
/* zk_d_pp_checked: zk_d_pp with the king's word checked.  The king of dist-primitives/src/dpp/mod.rs:37-52 receives
 * num ++ den per party and unpacks it with unpack_missing_shares: packed shares of degree < 2l, so the dimension is 2l and
 * up to (nparties - 2l) / 2 wrong shares per chunk are corrected.  num_d and den_d are [nparties][len] each, row i the shares
 * of parties[i] (NULL list: 0 .. nparties - 1), and are REPAIRED IN PLACE by two zk_pss_repair_parties calls; then the
 * unchecked king runs with the list.  Chunk c of the reference's word is num's chunk c for c < len and den's chunk c - len
 * above: status_d and errpos_d are [2 len] in that order, summary_d is [2][3 + n], num's then den's.  in_mask_d, out_mask_d
 * and out_d are [n][len] as in zk_d_pp.  The zero-denominator ZK_ERR_GENERIC is unchanged, and a den chunk that failed
 * (status 2: its shares go to the king as received) may cause it.  NOT CHECKED: the deg_red that ends d_pp (mod.rs:86) --
 * the king produced that word itself, and its cap is 0.  The refusals are those of the checked kings with a list above
 * (zk_d_pp's king reads its list the same way); len == 0 is ZK_OK. */
int zk_d_pp_checked(zk_ctx* ctx, void* num_d, void* den_d, const uint32_t* parties, int nparties, const void* in_mask_d,
                    const void* out_mask_d, size_t len, uint64_t seed, void* out_d, uint8_t* status_d, uint32_t* errpos_d,
                    uint64_t* summary_d, void* stream);
/* zk_pss_unpack_points_robust: the robust unpack of packed POINT shares -- the CRS vectors a party holds and the words the
 * d_msm kings receive are Reed-Solomon words over the share domain H_n whose symbols are curve points, Y_p = y_p G.
 * secret-sharing/src/pss.rs:125-166 with T = a group element; the code is that of secret-sharing/src/gao.rs, the decoder is
 * not: gao.rs divides polynomials by their coefficients, and there is no division in the exponent.  What can be formed are
 * fixed scalar combinations of the shares: the syndromes S_j = sum_p w_n^(-p j) Y_p, j = dimension .. n - 1, which are all the
 * identity exactly for a codeword, and which for ONE wrong share, E at party q, are S_j = w_n^(-q j) E -- q is the one
 * candidate with S_(j+1) = w_n^(-q) S_j, the honest share is Y_q - w_n^(q dimension) S_dimension.
 * CORRECTION CAPACITY: cap = 1 when n - dimension >= 2, cap = 0 when n - dimension = 1.  This is deliberately below gao.rs's
 * (n - dimension) / 2: locating e errors without division means trying error sets, C(n, e) of them with a linear system
 * each, and that does not scale to l = 8 (n = 32); one error is the model of the checked king rounds, one lying party.
 *   status 0  all syndromes are the identity.  out_d is zk_pss_unpack_points' result at dimension <= 2l and
 *             zk_pss_unpack2_points' above, byte for byte (affine output is canonical)
 *   status 1  exactly one share differs from a codeword of that dimension: errpos has that one bit, out_d is the unpack of
 *             the corrected word
 *   status 2  anything else: out_d is identities, errpos is 0.  For l >= 2 two to 2l - 1 wrong shares are always status 2
 *             (minimum distance 2l + 1 at dimension 2l); for l = 1 two wrong shares can lie within one of another codeword,
 *             the caveat of zk_pss_unpack_robust
 * summary_d is laid out as zk_pss_unpack_robust's.  shares_d is [n][nchunks] affine in party order, out_d [nchunks][l] affine.
 * PRECONDITION: every share is on the curve and in the order-r subgroup (zk_points_decompress_checked /
 * zk_points_subgroup_check establish it for wire input).  Outside it the verdicts mean nothing; the kernels still terminate,
 * every loop has a fixed trip count.
 * Errors: a bad group, a dimension outside 1 .. n - 1, or NULL shares_d / status_d with nchunks > 0 -> ZK_ERR_BAD_INPUT (the
 * context stays usable); nchunks == 0 is ZK_OK.  No host synchronisation inside the call, working memory from the stream's
 * workspace (the unpack matrix is the cached one of zk_pss_unpack_points).  All n parties only.  Device engine only. */
int zk_pss_unpack_points_robust(zk_ctx* ctx, int group, const void* shares_d /* [n][nchunks] affine */, size_t nchunks,
                                int dimension, void* out_d /* [nchunks][l] affine, or NULL */,
                                uint8_t* status_d /* [nchunks] */, uint32_t* errpos_d /* [nchunks], or NULL */,
                                uint64_t* summary_d /* [3 + n], or NULL */, void* stream);
/* zk_pss_repair_points: the verdicts of zk_pss_unpack_points_robust written back into the shares (pss.rs:125-166 over group
 * elements, gao.rs's code).  status_d, errpos_d, summary_d and the error returns are exactly that call's on the same input.
 * WRITTEN: in a status-1 chunk the one element errpos names becomes Y_q - E, in affine form.  NOT WRITTEN: anything else --
 * clean chunks, failed chunks, the other shares of a corrected chunk.  A second call finds the former status-1 chunks clean.
 * All n parties only.  No host synchronisation, working memory from the stream's workspace.  Device engine only. */
int zk_pss_repair_points(zk_ctx* ctx, int group, void* shares_d /* [n][nchunks] affine, in place */, size_t nchunks,
                         int dimension, uint8_t* status_d /* [nchunks] */, uint32_t* errpos_d /* [nchunks], or NULL */,
                         uint64_t* summary_d /* [3 + n], or NULL */, void* stream);
/* zk_pss_unpack_points_robust_parties: zk_pss_unpack_points_robust when only the listed parties' shares are at hand (a
 * party that was named before, or one that never answered, is left out).  shares_d is the compact [nparties][nchunks], row i
 * the shares of parties[i]; parties is a HOST list of ascending ids below n, NULL for 0 .. nparties - 1.  With S the listed
 * parties, rho = n - nparties and Lambda(X) = prod over the absent a of (X - w_n^a), the word Lambda(w_n^p) Y_p on S, the
 * identity elsewhere, has dimension `dimension + rho` on the full domain: the syndromes are
 * S_j = sum_{p in S} Lambda(w_n^p) w_n^(-p j) Y_p, j = dimension + rho .. n - 1 -- nparties - dimension of them, all the identity
 * exactly for a codeword -- and one wrong share E at a listed q gives S_(j+1) = w_n^(-q) S_j and
 * E = Lambda(w_n^q)^(-1) w_n^(q (dimension + rho)) S_(dimension + rho).  The factors of Lambda sit in the scalars, no share
 * is multiplied on its own.  CORRECTION CAPACITY: cap = 1 when nparties - dimension >= 2, cap = 0 when it is 1.
 * status, errpos and summary_d mean what they mean in zk_pss_unpack_points_robust with nparties in place of n: errpos and
 * the summary's per-party counts go by party ID, and an absent party is never named (a ratio that points at one is status 2).
 * out_d is the l secrets through the Lagrange matrix of the listed points (pss.rs:170-221), which is exact for any word of
 * dimension <= nparties; an absent party's share is not recovered.
 * PROMISED EQUAL: with nparties == n every output and every byte written equals zk_pss_unpack_points_robust's; on a clean
 * chunk out_d equals zk_pss_unpack2_points' with the same list wherever that call accepts the list, byte for byte (affine
 * output is canonical).  The PRECONDITION on the shares is that call's.
 * Errors, in this order: nparties outside 1 .. n, a list that is not strictly ascending or holds an id >= n, a dimension
 * outside 1 .. n - 1, a bad group, NULL shares_d / status_d with nchunks > 0 -> ZK_ERR_BAD_INPUT; nparties <= dimension ->
 * ZK_ERR_PROTOCOL, as zk_pss_unpack_robust_parties; then nchunks == 0 is ZK_OK.  The context stays usable after each.
 * The scalars of a (list, dimension) are computed on the host per new pair and their device copy is cached; after that no
 * host synchronisation.  Working memory from the stream's workspace.  Device engine only. */
int zk_pss_unpack_points_robust_parties(zk_ctx* ctx, int group, const void* shares_d /* [nparties][nchunks] affine */,
                                        const uint32_t* parties /* host, ascending, NULL = 0..nparties-1 */, int nparties,
                                        size_t nchunks, int dimension, void* out_d /* [nchunks][l] affine, or NULL */,
                                        uint8_t* status_d /* [nchunks] */, uint32_t* errpos_d /* [nchunks], or NULL */,
                                        uint64_t* summary_d /* [3 + n], or NULL */, void* stream);
/* zk_pss_repair_points_parties: the verdicts of zk_pss_unpack_points_robust_parties written back into the compact shares.
 * status_d, errpos_d, summary_d and the error returns are exactly that call's on the same input.  WRITTEN: in a status-1 chunk
 * the one element errpos names, at row i of parties[i], becomes Y_q - E in affine form.  NOT WRITTEN: anything else; an
 * absent party's share is not recovered.  A second call finds the former status-1 chunks clean.  With nparties == n every
 * byte written equals zk_pss_repair_points'. */
int zk_pss_repair_points_parties(zk_ctx* ctx, int group, void* shares_d /* [nparties][nchunks] affine, in place */,
                                 const uint32_t* parties, int nparties, size_t nchunks, int dimension,
                                 uint8_t* status_d /* [nchunks] */, uint32_t* errpos_d /* [nchunks], or NULL */,
                                 uint64_t* summary_d /* [3 + n], or NULL */, void* stream);
/* zk_d_msm_checked: zk_d_msm with the king's word checked.  The word is c_p = msm_p + in_mask_p
 * (dist-primitives/src/dmsm/mod.rs:73-85), of degree up to 4l - 2: dimension 4l - 1, one syndrome, sum_p w_n^p c_p --
 * DETECTION ONLY, as zk_deg_red_checked.  *status (HOST, one byte) is 0 when the syndrome is the identity and 2 otherwise;
 * `out` is written by zk_d_msm itself and never touched again: the same n group elements for the same input (Jacobian
 * coordinates are not canonical, and two zk_d_msm calls on one input need not agree in their bytes).  The syndrome is a second fused MSM over the same bases
 * and scalars with the coefficients w_n^p, so the call costs two zk_d_msm.  NULL status -> ZK_ERR_BAD_INPUT; the other
 * errors are zk_d_msm's.  There is no party-list form: with n - 1 parties no redundancy is left.  Device engine only. */
int zk_d_msm_checked(zk_ctx* ctx, int group, const void* bases_d, const void* scalars_d, size_t len, const void* in_mask,
                     const void* out_mask, void* out, uint8_t* status /* host, 1 byte */, void* stream);
/* zk_pss_repair_batch: zk_pss_repair of several share matrices the way a batched king takes them -- item i is a matrix
 * [n][nchunks] at shares_d + i * item_stride elements (the three words of a king round of circom_h, ext_wit.rs:127-170, lie
 * like this).  secret-sharing/src/gao.rs:47-84 per chunk, as zk_pss_repair.  status_d, errpos_d and summary_d follow
 * zk_pss_repair's definitions per item, the shares of an item change only where zk_pss_repair would change them, elements
 * between the items keep their bytes, and with nitems == 1 every output equals zk_pss_repair's byte for byte.
 * One clear, one scan launch and one decoder launch serve all items: a single call's fixed cost, not nitems of them.
 * Errors (ZK_ERR_BAD_INPUT, nothing written): nitems outside 1 .. 48, item_stride < n * nchunks,
 * nitems * nchunks >= 2^32, and the refusals of zk_pss_repair.  nchunks == 0 is ZK_OK.
 * All n parties only.  No host synchronisation, working memory from the stream's workspace.  Device engine only. */
int zk_pss_repair_batch(zk_ctx* ctx, void* shares_d /* in place */, size_t item_stride /* elements */, int nitems,
                        size_t nchunks, int dimension, uint8_t* status_d /* [nitems][nchunks] */,
                        uint32_t* errpos_d /* [nitems][nchunks], or NULL */,
                        uint64_t* summary_d /* [nitems][3 + n], or NULL */, void* stream);
/* zk_circom_h_checked: zk_circom_h with every word a king receives checked (groth16/src/ext_wit.rs:104-181; the kings
 * dist-primitives/src/dfft/mod.rs:264-304 and utils/deg_red.rs:99-115).  Seven words, in this order of items:
 *   0..2  the d_ifft words of a, b, c (ext_wit.rs:127-159): fft1(x) / m + in_mask; without an in-mask fft1(x), with the
 *         1 / m in the king's table -- the words of zk_d_ifft_checked
 *   3..5  the d_fft words (ext_wit.rs:161-170): fft1(x) + in_mask -- the words of zk_d_fft_checked
 *   6     the deg_red word (ext_wit.rs:173-179): a*b - c + in_mask at dimension 4l - 1 -- DETECTION ONLY as in
 *         zk_deg_red_checked: status 0 or 2, errpos 0, nothing rewritten
 * Items 0..5 have dimension 2l: up to l wrong parties per chunk are named and corrected, and h_share_d is then the honest
 * h.  The three words of a round are repaired by one zk_pss_repair_batch.  status_d and errpos_d are [7][m/l], summary_d
 * [7][3 + n], each item's as zk_pss_repair defines it.  On honest input h_share_d equals zk_circom_h's bit for bit under the
 * same seed and masks and every status is 0.  A failed chunk is no error return: its shares go to the king as received and
 * the item's summary_d[2] counts it.  The in-masks of a round may be partly present.
 * Errors: those of zk_circom_h, and a NULL status_d -> ZK_ERR_BAD_INPUT.  Device engine only. */
int zk_circom_h_checked(zk_ctx* ctx, const void* qap_a_d, const void* qap_b_d, const void* qap_c_d, int log2_m,
                        const zk_groth16_masks* masks, uint64_t seed, void* h_share_d, uint8_t* status_d /* [7][m/l] */,
                        uint32_t* errpos_d /* [7][m/l], or NULL */, uint64_t* summary_d /* [7][3 + n], or NULL */,
                        void* stream);
/* zk_groth16_prove_checked: zk_groth16_prove (groth16/src/prove.rs, examples/sha256.rs:32-129) with h computed by the chain
 * of zk_circom_h_checked on the prover's own stream and work buffers; everything else -- the MSMs, the host terms, the
 * assembly -- is zk_groth16_prove's.  Synchronous: when the call returns the proof is on the host and the report buffers
 * status_d / errpos_d / summary_d (device, the [7] layouts above) are complete.
 * COVERED: the seven king words of circom_h.  A party whose QAP shares or round-2 in-mask rows are wrong -- up to l of them
 * per chunk -- is named, and the proof is the honest proof.
 * NOT COVERED: the five d_msm rounds.  Their word has dimension 4l - 1, so checking them is detection only and costs a
 * second MSM each (zk_d_msm_checked); a caller who wants that calls it.  The async form is
 * zk_groth16_prove_checked_async, the batch form zk_groth16_prove_checked_batch.
 * Errors: those of zk_groth16_prove, and a NULL status_d -> ZK_ERR_BAD_INPUT. */
int zk_groth16_prove_checked(zk_ctx* ctx, const zk_crs_share* crs, const void* qap_a_d, const void* qap_b_d,
                             const void* qap_c_d, const void* a_share_d, const void* ax_share_d, const void* r, const void* s,
                             int log2_m, const zk_groth16_masks* masks, uint64_t seed, void* pi_a, void* pi_b, void* pi_c,
                             uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d, void* stream);
/* zk_pss_repair_batch_parties: zk_pss_repair_batch for the shares of ONE party list S, shared by all items -- the three words
 * of a king round when only the listed parties' words arrived (ext_wit.rs:127-170 with the list of unpack_missing_shares,
 * secret-sharing/src/pss.rs:141-221; gao.rs:11-84 over the points of S per chunk).  Item i is a COMPACT matrix
 * [nparties][nchunks] at shares_d + i * item_stride elements, row r the shares of parties[r], as zk_pss_repair_parties lays
 * them out; item_stride >= nparties * nchunks.  parties (HOST) holds ascending ids below n, NULL stands for
 * 0 .. nparties - 1.  status_d and errpos_d (by party id) are [nitems][nchunks], summary_d is [nitems][3 + n]; each follows
 * zk_pss_repair_parties' definitions per item, an item changes only where that call would change it, elements between the
 * items keep their bytes.  With nitems == 1 every output and byte written equals zk_pss_repair_parties', with nparties == n
 * zk_pss_repair_batch's.  One clear, the two tables of the list (once per call), one scan launch and one decoder launch
 * serve all items.
 * Errors (nothing written): a bad list or dimension -> ZK_ERR_BAD_INPUT and nparties <= dimension -> ZK_ERR_PROTOCOL as in
 * zk_pss_repair_parties; nitems outside 1 .. 48, item_stride < nparties * nchunks, nitems * nchunks >= 2^32, NULL shares_d
 * or status_d -> ZK_ERR_BAD_INPUT as in zk_pss_repair_batch.  nchunks == 0 is ZK_OK.
 * No host synchronisation, working memory from the stream's workspace.  Device engine only. */
int zk_pss_repair_batch_parties(zk_ctx* ctx, void* shares_d /* in place */,
                                const uint32_t* parties /* host, ascending ids, NULL = 0..nparties-1 */, int nparties,
                                size_t item_stride /* elements */, int nitems, size_t nchunks, int dimension,
                                uint8_t* status_d /* [nitems][nchunks] */, uint32_t* errpos_d /* [nitems][nchunks], or NULL */,
                                uint64_t* summary_d /* [nitems][3 + n], or NULL */, void* stream);
/* zk_circom_h_checked_parties: zk_circom_h_checked when only the listed parties' words reach the kings
 * (groth16/src/ext_wit.rs:104-181; the kings dist-primitives/src/dfft/mod.rs:264-304 and utils/deg_red.rs:99-115 with the list
 * of unpack_missing_shares, pss.rs:141-221) -- a dropout, or a party left out because an earlier report named it.  The list
 * is read and refused as the checked kings with a list read it, before anything is written: all n parties or n - 1 of them;
 * a malformed list is ZK_ERR_BAD_INPUT, a shorter one ZK_ERR_PROTOCOL.  With nparties == n this is zk_circom_h_checked.
 * The inputs and masks keep their [n][m/l] layouts.  The rows of an absent party in qap_*, in the six fft in-masks and in
 * degred_in have NO INFLUENCE on any output (they are not read).
 *   items 0..5  the words of the listed parties, compact, repaired by one zk_pss_repair_batch_parties of 3 items per round
 *               at dimension 2l (cap = (nparties - 2l) / 2 wrong parties per chunk, named by party id); the kings run with
 *               the list
 *   item 6      NOT CHECKED with n - 1 parties: at dimension 4l - 1 no redundancy is left.  The word goes to deg_red with
 *               the list as received; its status_d and errpos_d bytes are written 0 and its summary_d row is ALL ZEROS --
 *               zero chunks checked, which a clean item (summary [m/l, 0, 0, ..]) never shows
 * On honest input h_share_d equals zk_circom_h's bit for bit under the same seed and masks (the kings' randomness depends on
 * the seed only).  With a liar left out h_share_d is the honest h, items 0..5 report clean and no chunk reaches the decoder.
 * Errors: those of zk_circom_h_checked.  Device engine only. */
int zk_circom_h_checked_parties(zk_ctx* ctx, const uint32_t* parties /* host, ascending ids, NULL = 0..nparties-1 */,
                                int nparties, const void* qap_a_d, const void* qap_b_d, const void* qap_c_d, int log2_m,
                                const zk_groth16_masks* masks, uint64_t seed, void* h_share_d,
                                uint8_t* status_d /* [7][m/l] */, uint32_t* errpos_d /* [7][m/l], or NULL */,
                                uint64_t* summary_d /* [7][3 + n], or NULL */, void* stream);
/* zk_groth16_prove_checked_parties: zk_groth16_prove_checked with the party list carried through the whole proof
 * (groth16/src/prove.rs, examples/sha256.rs:32-129; the kings' unpack_missing_shares, pss.rs:141-221, and the d_msm king,
 * dist-primitives/src/dmsm/mod.rs:73-102, over the surviving parties as mpc-net/src/ser_net.rs:57-94 delivers them).  A
 * caller who has read a report asks with it for the honest proof from the remaining n - 1 parties.
 *   h chain     zk_circom_h_checked_parties with the list; the report buffers as there (item 6 NOT CHECKED with n - 1)
 *   MSM rounds  the five d_msm rounds and the host in-mask terms use the list's king coefficients (those of
 *               zk_d_msm_parties), zero at the absent party; every launch keeps the shape it has in zk_groth16_prove
 * CONTRACT: the absent party's rows of qap_*, a_share_d, ax_share_d and of every in-mask have no influence on the proof.
 * They must still be readable memory, field rows must hold field elements and point rows curve points: the MSM may read
 * them under a zero coefficient.  The MSM rounds stay UNCHECKED as in zk_groth16_prove_checked: a wrong a_share / ax_share
 * row of a LISTED party still spoils the proof.  The list is read and refused as zk_circom_h_checked_parties reads it,
 * before anything is written; with nparties == n this is zk_groth16_prove_checked.  Synchronous (the async form is
 * zk_groth16_prove_checked_parties_async); there is no batch or zk_dist_* form, no list for point shares, and the absent
 * party's share is not recovered.
 * Errors: those of zk_groth16_prove_checked and of the list. */
int zk_groth16_prove_checked_parties(zk_ctx* ctx, const uint32_t* parties /* host, ascending ids, NULL = 0..nparties-1 */,
                                     int nparties, const zk_crs_share* crs, const void* qap_a_d, const void* qap_b_d,
                                     const void* qap_c_d, const void* a_share_d, const void* ax_share_d, const void* r,
                                     const void* s, int log2_m, const zk_groth16_masks* masks, uint64_t seed, void* pi_a,
                                     void* pi_b, void* pi_c, uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d,
                                     void* stream);
/* zk_circom_h_batch_checked: zk_circom_h_checked for nproofs (1..16) proofs as ONE launch chain -- what a proving service
 * gets from the reference by running ext_wit.rs:104-181 once per concurrent dsha256 run (mpc-net/src/multi.rs:317-327), with
 * every king word of every proof checked.  CONTRACT: proof b is zk_circom_h_checked with seed + 16 b -- the same seven words,
 * dimensions (2l for items 0..5, 4l - 1 detection only for item 6) and verdicts; h_share_d is [nproofs][n][m/l].  The
 * report is PROOF-MAJOR: status_d and errpos_d [nproofs][7][m/l], summary_d [nproofs][7][3 + n]; the slice of proof b holds
 * what that single call writes, byte for byte, so one proof's report is handed out without reshuffling.  Pointer arrays are
 * host arrays of device pointers; masks: nproofs entries or NULL.  A round of the whole batch is one word launch, ONE
 * zk_pss_repair_batch of 3 nproofs items (48 at most: the item limit of that call) and one king launch; the report rows
 * are gathered to their proof-major places by the last launch of the chain.  When the in-masks of a stage are not present
 * or absent alike across the batch and a round's three words, the proofs run one by one: the same results.
 * Errors (ZK_ERR_BAD_INPUT, nothing written): nproofs outside 1 .. 16, NULL pointers (arrays, entries, h_share_d,
 * status_d), 3 nproofs m/l >= 2^32, and everything zk_circom_h_checked refuses.  A failed chunk is no error return.
 * No host synchronisation.  Device engine only. */
int zk_circom_h_batch_checked(zk_ctx* ctx, int nproofs, const void* const* qap_a_d, const void* const* qap_b_d,
                              const void* const* qap_c_d, int log2_m, const zk_groth16_masks* masks, uint64_t seed,
                              void* h_share_d /* [nproofs][n][m/l] */, uint8_t* status_d /* [nproofs][7][m/l] */,
                              uint32_t* errpos_d /* [nproofs][7][m/l], or NULL */,
                              uint64_t* summary_d /* [nproofs][7][3 + n], or NULL */, void* stream);
/* Asynchronous forms of zk_groth16_prove_checked and zk_groth16_prove_checked_parties (what `tokio::spawn(dsha256(..))` is to
 * the reference, mpc-net/src/multi.rs:317-327, with the kings' words checked): the arguments of the synchronous calls
 * without the proof outputs; the handle is one of zk_groth16_prove_async's -- zk_groth16_wait joins it and writes the
 * shares, zk_groth16_abort frees the slot, two proofs of either kind may be in flight.  The report buffers are complete when
 * zk_groth16_wait returns.  `parties` is read before the call returns and may be freed or overwritten at once; every other
 * input must stay valid until the join, as for zk_groth16_prove_async.  The synchronous calls are these followed by
 * zk_groth16_wait. */
int zk_groth16_prove_checked_async(zk_ctx* ctx, const zk_crs_share* crs, const void* qap_a_d, const void* qap_b_d,
                                   const void* qap_c_d, const void* a_share_d, const void* ax_share_d, const void* r,
                                   const void* s, int log2_m, const zk_groth16_masks* masks, uint64_t seed, uint8_t* status_d,
                                   uint32_t* errpos_d, uint64_t* summary_d, void* stream, int* handle);
int zk_groth16_prove_checked_parties_async(zk_ctx* ctx, const uint32_t* parties /* host, ascending ids, NULL = 0..nparties-1 */,
                                           int nparties, const zk_crs_share* crs, const void* qap_a_d, const void* qap_b_d,
                                           const void* qap_c_d, const void* a_share_d, const void* ax_share_d, const void* r,
                                           const void* s, int log2_m, const zk_groth16_masks* masks, uint64_t seed,
                                           uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d, void* stream,
                                           int* handle);
/* zk_groth16_prove_checked_batch: zk_groth16_prove_batch (concurrent dsha256 runs, groth16/examples/sha256.rs:316-360) with
 * h computed by the chain of zk_circom_h_batch_checked on the batch's own stream and work buffers; the report buffers
 * (device) in that call's proof-major layout.  Proof b is the proof zk_groth16_prove_checked gives with seed + 16 b, as
 * group elements.  The five d_msm rounds stay UNCHECKED as in the single call.  There is no party list for a batch.
 * _async returns a handle of zk_groth16_prove_batch_async's space: zk_groth16_batch_wait joins it, after which the report
 * is complete; checked and unchecked batches may be in flight together, three in all, each with its own scratch.
 * Errors: those of zk_groth16_prove_batch, and a NULL status_d -> ZK_ERR_BAD_INPUT. */
int zk_groth16_prove_checked_batch(zk_ctx* ctx, const zk_crs_share* crs, int nproofs, const void* const* qap_a_d,
                                   const void* const* qap_b_d, const void* const* qap_c_d, const void* const* a_share_d,
                                   const void* const* ax_share_d, const void* r, const void* s, int log2_m,
                                   const zk_groth16_masks* masks, uint64_t seed, void* pi_a, void* pi_b, void* pi_c,
                                   uint8_t* status_d /* [nproofs][7][m/l] */, uint32_t* errpos_d /* or NULL */,
                                   uint64_t* summary_d /* [nproofs][7][3 + n], or NULL */, void* stream);
int zk_groth16_prove_checked_batch_async(zk_ctx* ctx, const zk_crs_share* crs, int nproofs, const void* const* qap_a_d,
                                         const void* const* qap_b_d, const void* const* qap_c_d,
                                         const void* const* a_share_d, const void* const* ax_share_d, const void* r,
                                         const void* s, int log2_m, const zk_groth16_masks* masks, uint64_t seed,
                                         uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d, void* stream,
                                         int* handle);
int zk_fr_to_bytes(zk_ctx* ctx, const void* x_d, size_t len, void* bytes_out_d, void* stream);
int zk_fr_from_bytes(zk_ctx* ctx, const void* bytes_d, size_t len, void* x_out_d, void* stream);
/* Vectors of group elements in ark-serialize's COMPRESSED form (what CRS shares / MSM results look like on an mpc-net
 * wire, ser_net.rs:111-120) <-> affine Montgomery points on the device: len x (|Fq| bytes for G1, 2 |Fq| for G2).
 * BN254 / BLS12-377: ark-ec's default flags (little-endian x, bit 7 / 6 of the last byte = y is the larger root /
 * infinity); BLS12-381: the zcash encoding ark-bls12-381 uses (big-endian, c1 || c0, flags in the first byte).
 * Decompression tests what arkworks tests before its subgroup test: x below the modulus, a y on the curve, consistent
 * flags.  It does NOT test membership in the order-r subgroup, which deserialize_compressed (Validate::Yes) also does:
 * zk_points_decompress_checked below is the call with that test.  It returns ZK_ERR_GENERIC naming the first bad index.  Square roots: the (q + 1) / 4 power for q = 3 mod 4 (BN254, BLS12-381),
 * Tonelli-Shanks for BLS12-377 (q - 1 = 2^46 t). */
int zk_points_decompress(zk_ctx* ctx, int group, const void* bytes_d, size_t len, void* out_affine_d, void* stream);
int zk_points_compress(zk_ctx* ctx, int group, const void* affine_d, size_t len, void* bytes_out_d, void* stream);
/* libsnark_h (ext_wit.rs:14-102) for all parties on this device: fft_in / fft_out: 7 mask pointers each ([n][m/l]
 * device buffers, NULL entries or NULL arrays = FftMask::zero) in the order 3 x d_ifft, 3 x d_fft, final d_ifft. */
int zk_libsnark_h(zk_ctx* ctx, const void* qap_a_d, const void* qap_b_d, const void* qap_c_d, int log2_m,
                  const void* const* fft_in, const void* const* fft_out, uint64_t seed, void* h_d, void* stream);
/* The five zk_d_msm_local of the prover for this rank's parties, overlapped: _begin starts S, H, V, W (they only
 * need the witness shares; crs vectors are [nparties][len] here) on internal streams and returns; _finish runs U
 * on `stream` once h_share_d [nparties][m/l] is available, joins, and writes out[0..4] = S, H, V(G2), W, U
 * (Jacobian, host).  skip_h != 0 when r = 0 (prove.rs:96-98).  masks (optional): msm_in[k] = this rank's nparties
 * in-mask points of MSM k (the other members are ignored here).  The internal streams wait for everything already
 * queued on `stream` (the shares may still be in flight there).  crs must stay valid until _finish returns. */
int zk_groth16_msms_begin(zk_ctx* ctx, const zk_crs_share* crs, const void* a_share_d, const void* ax_share_d,
                          int first_party, int nparties, int skip_h, const zk_groth16_masks* masks, void* stream);
int zk_groth16_msms_finish(zk_ctx* ctx, const void* h_share_d, void* const* out, void* stream);
/* Asynchronous form of zk_groth16_prove (what `tokio::spawn(dsha256(..))` is to the reference, multi.rs:317-327):
 * _async enqueues the whole proof -- device pipelines on internal streams, host-side terms on the context's worker
 * pool -- and returns a handle without waiting; _wait joins and writes the shares.  Up to two proofs may be in
 * flight per context (each has its own scratch); inputs must stay valid and unmodified until _wait returns.
 * _abort joins and discards a proof in flight (also safe after a failed call); it also releases a handle handed out
 * by zk_dist_groth16_prove_async (same handle space), which every rank must then abort alike. */
int zk_groth16_prove_async(zk_ctx* ctx, const zk_crs_share* crs, const void* qap_a_d, const void* qap_b_d,
                           const void* qap_c_d, const void* a_share_d, const void* ax_share_d, const void* r,
                           const void* s, int log2_m, const zk_groth16_masks* masks, uint64_t seed, void* stream,
                           int* handle);
int zk_groth16_wait(zk_ctx* ctx, int handle, void* pi_a, void* pi_b, void* pi_c);
int zk_groth16_abort(zk_ctx* ctx, int handle);
int zk_groth16_assemble(zk_ctx* ctx, const zk_crs_share* crs, const void* r, const void* s, const void* const* sums,
                        const zk_groth16_masks* masks, void* pi_a, void* pi_b, void* pi_c);
/* A BATCH of proofs against one packed CRS in one pass -- what a proving service does with the reference by spawning
 * concurrent dsha256 runs (mpc-net/src/multi.rs:317-327 runs the parties as concurrent tasks; groth16/examples/
 * sha256.rs:316-360 is one such run): nproofs (1..16) witnesses, each with its own QAP shares, witness shares, (r, s)
 * and masks, same CRS and domain.  Every one of the five d_msm is ONE sort / accumulate / reduce chain over nproofs
 * scalar vectors against the shared base vector, circom_h one launch chain over 3 nproofs vectors; the results are the
 * group elements nproofs calls of zk_groth16_prove give.  Pointer arrays are host arrays of device pointers; r, s:
 * nproofs Montgomery Fr each (host, contiguous); masks: nproofs entries or NULL; pi_a / pi_c: [nproofs][n] Jacobian G1,
 * pi_b: [nproofs][n] Jacobian G2 (host).  Replay mode: proof b draws the share randomness zk_groth16_prove draws with
 * seed + 16 b. */
int zk_groth16_prove_batch(zk_ctx* ctx, const zk_crs_share* crs, int nproofs, const void* const* qap_a_d,
                           const void* const* qap_b_d, const void* const* qap_c_d, const void* const* a_share_d,
                           const void* const* ax_share_d, const void* r, const void* s, int log2_m,
                           const zk_groth16_masks* masks, uint64_t seed, void* pi_a, void* pi_b, void* pi_c, void* stream);
/* Asynchronous form: _async enqueues the batch (device pipelines on the batch's own stream set, host terms on the worker
 * pool) and returns a handle; zk_groth16_batch_wait joins it and writes the shares.  Up to THREE batches may be in flight
 * per context, each with its own scratch: the sorts of one run under the accumulate kernels of the other (two already
 * saturate the chip: 814 / 813 proofs/s with two / three batches of 8 in flight).  Inputs must
 * stay valid and unmodified until _wait returns (the pointer ARRAYS are copied and may be reused at once). */
int zk_groth16_prove_batch_async(zk_ctx* ctx, const zk_crs_share* crs, int nproofs, const void* const* qap_a_d,
                                 const void* const* qap_b_d, const void* const* qap_c_d, const void* const* a_share_d,
                                 const void* const* ax_share_d, const void* r, const void* s, int log2_m,
                                 const zk_groth16_masks* masks, uint64_t seed, void* stream, int* handle);
int zk_groth16_batch_wait(zk_ctx* ctx, int handle, void* pi_a, void* pi_b, void* pi_c);
/* G::msm of ONE base vector bases_d [len] against nvec (1..16) scalar vectors scalars_d[v] [len] (dmsm/mod.rs:73 called
 * once per witness): one Pippenger pass with bucket sets per scalar vector.  out: nvec Jacobian points (host). */
int zk_msm_batch(zk_ctx* ctx, int group, const void* bases_d, size_t len, const void* const* scalars_d, int nvec,
                 void* out, void* stream);
/* sum_i G::msm(bases_d[i] [lens[i]], scalars_d[i] [lens[i]]) for k = 1..3 MSMs over one group, as ONE Jacobian point (host).
 * Bucket accumulation is linear: the launches whose bucket geometry (window bits and count, bucket sets, buckets per set:
 * equal for vectors registered with the same table width, or table-free vectors of lengths the cost model gives the same
 * window) equals the LAST vector's stop behind their bucket sums, the last launch adds their buckets to its own and ONE
 * bucket set is reduced and folded for all of them; the others are reduced on their own and added on the host.  The full
 * prover ends r*H + W + U this way.  shared (optional): how many of the first k - 1 launches shared the last one's set. */
int zk_msm_sum(zk_ctx* ctx, int group, int k, const void* const* bases_d, const void* const* scalars_d, const size_t* lens,
               void* out, int* shared, void* stream);
/* unpack / unpack2 over GROUP elements (secret-sharing/src/pss.rs:125-166 with T = curve point; lagrange_unpack
 * :170-221 for a party subset): shares_d [nparties][nchunks] affine points of the listed parties (ascending ids, NULL =
 * 0..nparties-1) -> out_d [nchunks][l] affine.  zk_pss_unpack_points needs all n parties. */
int zk_pss_unpack_points(zk_ctx* ctx, int group, const void* shares_d, size_t nchunks, void* out_d, void* stream);
int zk_pss_unpack2_points(zk_ctx* ctx, int group, const void* shares_d, const uint32_t* parties, int nparties,
                          size_t nchunks, void* out_d, void* stream);
/* The last step of the reference's run (groth16/examples/sha256.rs:375-377): (a, b, c) = pp.unpack2(shares)[0] over the
 * parties' proof shares.  pi_a / pi_c: nparties Jacobian G1, pi_b: nparties Jacobian G2 (host) of the listed parties
 * (ascending ids, NULL = all n; a subset goes through lagrange_unpack and needs more than 2 (t + l - 1) of them).
 * proof_affine (optional, host): A (G1) | B (G2) | C (G1) as affine Montgomery points; proof_bytes (optional, host):
 * ark_groth16::Proof::serialize_compressed, 4 |Fq| bytes (128 for BN254; BLS12-381: 192 in the zcash form). */
int zk_groth16_reconstruct(zk_ctx* ctx, const void* pi_a, const void* pi_b, const void* pi_c, const uint32_t* parties,
                           int nparties, void* proof_affine, void* proof_bytes, void* stream);

/* ---- the star network on one multi-GPU node (mpc-net/src/lib.rs:43-53, 89-176 `MpcNet`; ser_net.rs:16-120) -------
 * One process per GPU; rank rho drives k = n / world parties: with party_to_rank == NULL the block [rho*k, (rho+1)*k),
 * otherwise the parties p with party_to_rank[p] == rho (MpcNet ids are arbitrary, lib.rs:43-53; any map that gives every
 * rank k parties is accepted; a rank's rows are in ascending party order, zk_net_parties lists them).  The king's work is
 * done by rank 0.  The king kernels always see the present parties' rows in ascending party order: with a
 * non-contiguous map gather / scatter move party rows one by one, and the all-to-all king falls back to the star.
 * `sid` = MultiplexedStreamID: channels 0..2 may be in flight at once (ext_wit.rs:158-170), calls on one channel are
 * ordered (multi.rs:418-445); channel 3 is used internally by zk_dist_groth16_prove.
 * Transports: ZK_NET_RCCL (ncclSend / ncclRecv over xGMI on device buffers), ZK_NET_SHM (staged through POSIX shared
 * memory: tests, several ranks on one GPU; with ctx == NULL the buffers of the raw verbs are HOST memory),
 * ZK_NET_LOCAL (world = 1).
 * Timeouts (lib.rs:98-135, ser_net.rs:57-94,122-125): a rank that does not enter a round within the timeout (default
 * 30 s, zk_net_set_timeout_ms) is left out of it; the king continues with the remaining parties through
 * lagrange_unpack when enough remain (else ZK_ERR_PROTOCOL "Not enough shares"), the late rank's call returns
 * ZK_ERR_PROTOCOL with its first party id.  zk_dist_groth16_prove needs every party.
 * id: ZK_NET_ID_BYTES made by zk_net_unique_id on rank 0 and handed to every rank by the launcher. */
typedef struct zk_net zk_net;
enum zk_transport { ZK_NET_LOCAL = 0, ZK_NET_RCCL = 1, ZK_NET_SHM = 2 };
#define ZK_NET_ID_BYTES 512
int zk_net_unique_id(void* id_out);
int zk_net_create(zk_ctx* ctx, int transport, int rank, int world, int n_parties /* used when ctx == NULL */,
                  const int* party_to_rank, const void* id, size_t shm_bytes_per_channel, zk_net** out);
void zk_net_destroy(zk_net* net);
const char* zk_net_last_error(zk_net* net, int* party);
int zk_net_set_timeout_ms(zk_net* net, uint64_t ms);
int zk_net_info(const zk_net* net, int info[4]);          /* rank, world, first party, parties per rank */
int zk_net_parties(const zk_net* net, int rank, int* parties /* k ids, ascending */);
int zk_net_stats(const zk_net* net, uint64_t stats[4]);   /* since creation: gathers, scatters, all-to-alls, bytes this rank sent */
/* raw verbs (what the primitives below are made of; exposed for hosts that compose their own rounds).
 * zk_net_enter: join the next round on `sid`; *mask = ranks taking part.  gather = client_send_or_king_receive
 * (lib.rs:89-135): bytes_per_rank from every rank, the king's `full` receives the present ranks' blocks compacted in
 * rank order.  scatter = client_receive_or_king_send (:137-176): rank r receives block r of the king's `full`.
 * *_host move small host values (<= 4096 bytes) through the control block.  Transfers on a channel are enqueued on
 * the channel's stream; zk_net_sync waits for it with the timeout as deadline.
 * zk_net_alltoall (no counterpart in mpc-net, whose topology is a star: the exchange of the all-to-all king, option
 * "king_alltoall"): the block for rank r is read at send + r*bytes_per_peer (indexed by RANK), the block from the i-th
 * PRESENT rank lands at recv + i*bytes_per_peer (compacted, like gather).
 * Waiting: the zk_dist_* calls return with their device work enqueued and make the caller's stream wait for the channel
 * streams.  A host that wants the timeout to hold for the data plane as well (a peer that dies mid-round, a hung RCCL
 * collective) calls zk_net_sync(net, sid) BEFORE synchronising its own stream: zk_net_sync waits with the timeout as a
 * deadline, aborts the communicators on expiry and returns ZK_ERR_PROTOCOL; a plain stream synchronise would block
 * behind the hung collective forever.  After a PROTOCOL / NOT_CONNECTED result the net must be destroyed and rebuilt. */
int zk_net_enter(zk_net* net, int sid, uint32_t* mask);
int zk_net_gather(zk_net* net, int sid, uint32_t mask, const void* local, size_t bytes_per_rank, void* full);
int zk_net_scatter(zk_net* net, int sid, uint32_t mask, const void* full, size_t bytes_per_rank, void* local);
int zk_net_alltoall(zk_net* net, int sid, uint32_t mask, const void* send, size_t bytes_per_peer, void* recv);
int zk_net_gather_host(zk_net* net, int sid, uint32_t mask, const void* mine, size_t bytes, void* all);
int zk_net_bcast_host(zk_net* net, int sid, uint32_t mask, void* buf, size_t bytes);
int zk_net_sync(zk_net* net, int sid);

/* ---- the reference's entry points as they are CALLED there: per party (here: per rank = its k parties), with a net
 * and a stream id, collectively by all ranks.  Buffers hold THIS RANK's rows: shares [k][m/l], masks [k][m/l] (NULL =
 * the *::zero() mask), MSM masks / outputs k Jacobian points (host).
 *   d_fft(pd_shares, rearrange, &FftMask, pp, &net, sid)            dfft/mod.rs:99-134   -> zk_dist_d_fft
 *   d_ifft(pd_shares, rearrange, &FftMask, dom, g, pp, &net, sid)   dfft/mod.rs:137-175  -> zk_dist_d_ifft
 *   deg_red(px, pp, &DegRedMask, &net, sid)                         deg_red.rs:80-126    -> zk_dist_deg_red
 *   d_pp(num, den, &DegRedMask, pp, &net, sid)                      dpp/mod.rs:15-87     -> zk_dist_d_pp
 *   d_msm(bases, scalars, &MsmMask, pp, &net, sid)                  dmsm/mod.rs:59-102   -> zk_dist_d_msm
 *   circom_h(qap_share, pp, masks.., &net)  (channels 0..2)         ext_wit.rs:104-181   -> zk_dist_circom_h
 *   dsha256(pp, crs_share, qap_share, a_share, ax_share, .., &net)  sha256.rs:32-129     -> zk_dist_groth16_prove */
int zk_dist_d_fft(zk_ctx* ctx, zk_net* net, int sid, void* shares_d, const void* in_mask_d, const void* out_mask_d,
                  int rearrange, int log2_m, uint64_t seed, void* stream);
int zk_dist_d_ifft(zk_ctx* ctx, zk_net* net, int sid, void* shares_d, const void* in_mask_d, const void* out_mask_d,
                   int rearrange, int log2_m, const void* g, uint64_t seed, void* stream);
int zk_dist_deg_red(zk_ctx* ctx, zk_net* net, int sid, void* x_d, const void* in_mask_d, const void* out_mask_d,
                    size_t len, uint64_t seed, void* stream);
int zk_dist_d_pp(zk_ctx* ctx, zk_net* net, int sid, const void* num_d, const void* den_d, const void* in_mask_d,
                 const void* out_mask_d, size_t len, uint64_t seed, void* out_d, void* stream);
int zk_dist_d_msm(zk_ctx* ctx, zk_net* net, int sid, int group, const void* bases_d, const void* scalars_d, size_t len,
                  const void* in_mask, const void* out_mask, void* out, void* stream);
/* deg_red over GROUP elements per rank (dist-primitives/src/utils/deg_red.rs:80-126 is generic over T: DomainCoeff<F> = F or
 * G and takes net, sid): x_d, masks, out_d are this rank's k parties' rows [k][len] of affine points (out_d must not alias
 * x_d); gen_affine as in zk_deg_red_points.  A rank the round left out is handled like for field elements (the king's
 * unpack2 becomes the Lagrange form over the present parties). */
int zk_dist_deg_red_points(zk_ctx* ctx, zk_net* net, int sid, int group, const void* x_d, const void* in_mask_d,
                           const void* out_mask_d, size_t len, const void* gen_affine, uint64_t seed, void* out_d,
                           void* stream);
/* libsnark_h per rank (groth16/src/ext_wit.rs:14-102): three d_ifft with the coset shift F::GENERATOR joined on channels
 * 0..2, three d_fft likewise, (a b - c) / Z(g), d_ifft with g^-1 on channel 0.  qap_*_d, h_d and the seven masks
 * (arrays of 7 pointers, or NULL for FftMask::zero) are this rank's rows [k][m/l]. */
int zk_dist_libsnark_h(zk_ctx* ctx, zk_net* net, const void* qap_a_d, const void* qap_b_d, const void* qap_c_d, int log2_m,
                       const void* const* fft_in_masks, const void* const* fft_out_masks, uint64_t seed, void* h_d,
                       void* stream);
int zk_dist_circom_h(zk_ctx* ctx, zk_net* net, const void* qap_a_d, const void* qap_b_d, const void* qap_c_d, int log2_m,
                     const zk_groth16_masks* masks, uint64_t seed, void* h_d, void* stream);
int zk_dist_groth16_prove(zk_ctx* ctx, zk_net* net, const zk_crs_share* crs, const void* qap_a_d, const void* qap_b_d,
                          const void* qap_c_d, const void* a_share_d, const void* ax_share_d, const void* r, const void* s,
                          int log2_m, const zk_groth16_masks* masks, uint64_t seed, void* pi_a, void* pi_b, void* pi_c,
                          void* stream);

/* ---- checked king rounds on the net: the per-rank calls above with the word the king RECEIVES from the other ranks checked
 * before the king reads it -- the place where a lying party is another process (client_send_or_king_receive in
 * dist-primitives/src/dfft/mod.rs:264-304 and dist-primitives/src/utils/deg_red.rs:99-115).  Each takes the unchecked
 * call's arguments, then status_d [len], errpos_d [len] (or NULL) and summary_d [3 + n] (or NULL), all DEVICE pointers, the
 * same (NULL or not) on every rank.  The list is the parties of the ranks zk_net_enter admitted; it is refused as
 * zk_*_checked_parties refuse a list (all n parties or n - 1 of them, else ZK_ERR_PROTOCOL), before anything is written and
 * on every rank alike.
 *   WHERE THE REPORT LANDS  every present rank zeroes status_d / errpos_d on entry and then writes exactly the chunks it
 *   was king of: rank 0 all of them under the star king, each rank its range under the all-to-all king (option
 *   king_alltoall) -- the OR over the ranks is the single-device report.  summary_d is complete and IDENTICAL on every
 *   present rank and equals the summary of zk_*_checked[_parties] on the same word; it crosses the net on the round's own
 *   channel after the king.  A failed chunk is no error return: its shares go to the king as received.
 * With the LOCAL transport the results are zk_d_fft_checked's / zk_d_ifft_checked's / zk_deg_red_checked's.  With a
 * general party_to_rank map the all-to-all king does not apply and the checked calls use the star, as the unchecked do. */
/* d_fft(pd_shares, rearrange, &FftMask, pp, &net, sid), dfft/mod.rs:99-134, king :264-304: the word fft1(x) + in_mask at
 * dimension 2l, up to (nparties - 2l) / 2 wrong shares per chunk corrected */
int zk_dist_d_fft_checked(zk_ctx* ctx, zk_net* net, int sid, void* shares_d, const void* in_mask_d, const void* out_mask_d,
                          int rearrange, int log2_m, uint64_t seed, uint8_t* status_d, uint32_t* errpos_d,
                          uint64_t* summary_d, void* stream);
/* d_ifft(pd_shares, rearrange, &FftMask, dom, g, pp, &net, sid), dfft/mod.rs:137-175, king :264-304 */
int zk_dist_d_ifft_checked(zk_ctx* ctx, zk_net* net, int sid, void* shares_d, const void* in_mask_d, const void* out_mask_d,
                           int rearrange, int log2_m, const void* g, uint64_t seed, uint8_t* status_d, uint32_t* errpos_d,
                           uint64_t* summary_d, void* stream);
/* deg_red(px, pp, &DegRedMask, &net, sid), utils/deg_red.rs:80-126, king :99-115: dimension 4l - 1, DETECTION ONLY (a status is
 * 0 or 2, nothing is rewritten).  With a rank absent the n - 1 words leave no redundancy: NOT CHECKED -- status and errpos
 * bytes 0 and an all-zero summary, as item 6 of zk_circom_h_checked_parties. */
int zk_dist_deg_red_checked(zk_ctx* ctx, zk_net* net, int sid, void* x_d, const void* in_mask_d, const void* out_mask_d,
                            size_t len, uint64_t seed, uint8_t* status_d, uint32_t* errpos_d, uint64_t* summary_d,
                            void* stream);
/* circom_h(qap_share, pp, masks.., &net), groth16/src/ext_wit.rs:104-181: zk_dist_circom_h with its six transform rounds
 * (:127-170) and the deg_red round (:173-179) checked.  status_d / errpos_d [7][m/l], summary_d [7][3 + n], the items in the
 * order of zk_circom_h_checked; the three channels of a phase stay in flight together. */
int zk_dist_circom_h_checked(zk_ctx* ctx, zk_net* net, const void* qap_a_d, const void* qap_b_d, const void* qap_c_d,
                             int log2_m, const zk_groth16_masks* masks, uint64_t seed, void* h_d, uint8_t* status_d,
                             uint32_t* errpos_d, uint64_t* summary_d, void* stream);

/* The sharded prover in two halves (the reference's parties are concurrent tasks, mpc-net/src/multi.rs:317-327, and
 * prove.rs:209-227 joins the W and U d_msm): zk_dist_groth16_prove_async admits the proof, starts this rank's four witness
 * MSMs, runs circom_h's king rounds on channels 0..2 and queues the U-MSM behind them -- it returns with that work
 * enqueued; zk_dist_groth16_wait joins it, exchanges the five partial sums with the king on channel 3 and writes the k
 * proof shares.  Up to TWO proofs may be in flight per rank; every rank must issue the same sequence of calls (the
 * channels are ordered): async(A), async(B), wait(A), async(C), wait(B) ... overlaps a proof's king rounds with the
 * previous proof's MSMs.  zk_dist_groth16_prove = async + wait.  Shares stay valid until the wait; masks are read at
 * async time (the struct is copied, the rows it points to must stay valid until the wait). */
int zk_dist_groth16_prove_async(zk_ctx* ctx, zk_net* net, const zk_crs_share* crs, const void* qap_a_d, const void* qap_b_d,
                                const void* qap_c_d, const void* a_share_d, const void* ax_share_d, const void* r,
                                const void* s, int log2_m, const zk_groth16_masks* masks, uint64_t seed, void* stream,
                                int* handle);
int zk_dist_groth16_wait(zk_ctx* ctx, zk_net* net, int handle, void* pi_a, void* pi_b, void* pi_c);

/* Throughput mode of the sharded prover: nproofs (1..16) proofs per collective call -- what a service does with the
 * reference by running several dsha256 instances over one mesh (mpc-net/src/multi.rs:317-327; groth16/examples/
 * sha256.rs:316-360).  ONE round of the control plane admits the batch; every rank runs each of its five d_msm once
 * over the nproofs witnesses (zk_groth16_prove_batch's batched Pippenger) beside the king rounds of the proofs'
 * circom_h; the partial sums of the batch cross in one host message per rank.  Pointer arrays (host arrays of device
 * pointers) hold THIS RANK's rows of every proof; r, s: nproofs Montgomery Fr each; masks: nproofs entries (this rank's
 * rows) or NULL; pi_a / pi_c: [nproofs][k] Jacobian G1, pi_b: [nproofs][k] Jacobian G2 (host).  Results equal nproofs
 * calls of zk_dist_groth16_prove; in replay mode proof b draws the randomness of seed + 16 b. */
int zk_dist_groth16_prove_batch(zk_ctx* ctx, zk_net* net, const zk_crs_share* crs, int nproofs,
                                const void* const* qap_a_d, const void* const* qap_b_d, const void* const* qap_c_d,
                                const void* const* a_share_d, const void* const* ax_share_d, const void* r, const void* s,
                                int log2_m, const zk_groth16_masks* masks, uint64_t seed, void* pi_a, void* pi_b,
                                void* pi_c, void* stream);

/* ---- per-party entry points: ONE CALLER PER PARTY, as the reference calls its primitives ------------------------------
 * simulate_network_round (mpc-net/src/multi.rs:301-328) runs one task per party; each task calls d_fft / d_msm / dsha256
 * with its OWN share vector and its own net handle (dist-primitives/src/dfft/mod.rs:99-111, dmsm/mod.rs:59-66,
 * groth16/examples/sha256.rs:316-360).  A zk_party is that net handle: party `party_id` of the k = n / world parties this
 * rank drives.  Each zk_party_* call below is the rank call of the same name (zk_dist_d_fft ... zk_dist_groth16_prove)
 * issued ONCE per round with the k parties' rows, once all k parties of the rank are inside it: it returns what the rank
 * call returns, and each party's output is its row of the rank call's output.  The rank calls stay, and stay the fast path.
 *   EXECUTOR  the calls BLOCK in a rendezvous until the rank's other parties have arrived, so a host needs one thread per
 *             party that can be inside a call at once: k threads, times the channels it keeps open at once.  In an async
 *             runtime that means spawn_blocking, or at least that many worker threads.
 *   ROUNDS    per (net, sid) the k callers of a round must pass equal scalar arguments (log2_m, len, rearrange, seed, group,
 *             the bytes of g, r and s, the CRS lengths, and which pointers are NULL); otherwise all k get ZK_ERR_BAD_INPUT,
 *             zk_party_last_error names the lowest party that differs from the rank's first party, nothing has entered
 *             the net round and the net stays usable.  A party that does not arrive within the net's timeout
 *             (zk_net_set_timeout_ms) fails the round for the waiting parties with ZK_ERR_PROTOCOL and its id; the channel
 *             then refuses every later call at once, the rank has not entered the net round (the other ranks see a late
 *             rank), and the net must be rebuilt as after any PROTOCOL result.  Two threads inside the same (party, sid) at
 *             once: ZK_ERR_BAD_INPUT for the second.  Channels 0..2 may be in flight at once, each with its own rendezvous;
 *             zk_party_circom_h and zk_party_groth16_prove meet on channel 0 and use the channels their rank calls use.
 *   STREAMS   a caller's `stream` is its own.  The library records an event on it on arrival; an internal per-(net, sid)
 *             stream waits for the k events and carries the rank call; every caller's stream then waits for its completion
 *             event.  As with the rank calls, a call returns with its device work ENQUEUED; the only host waits are the
 *             rendezvous and whatever the rank call already waits for.
 *   ROWS      if the k pointers of an operand are the rows of one block (p[i] == p[0] + i * row_bytes, ascending party
 *             order) the rank call gets the first pointer and nothing is copied; registered fixed-base tables apply.
 *             Otherwise the operand is staged through a per-(net, sid) buffer (one gather launch, one scatter launch for
 *             in-place outputs); staged MSM bases never use a registered table.  A row that is not 16-byte aligned is
 *             ZK_ERR_BAD_INPUT.  k is at most 32.
 * zk_net_party: party_id not driven by this rank (or k > 32) -> ZK_ERR_BAD_INPUT.  Handles are released before their net is
 * destroyed.  A party may be driven through any number of handles, one after another (a handle per task is fine): the order
 * of its calls on a channel belongs to the party, not to a handle.  zk_party_last_error: per handle, so that k threads do not share one string.  zk_party_stats: rounds issued,
 * of them zero-copy, of them staged, bytes staged (both directions), since the net's first zk_net_party. */
typedef struct zk_party zk_party;
int zk_net_party(zk_net* net, int party_id, zk_party** out);
void zk_party_release(zk_party* p);
int zk_party_id(const zk_party* p);
const char* zk_party_last_error(zk_party* p, int* party);
int zk_party_stats(zk_net* net, uint64_t stats[4]);
/* d_fft(pd_shares, rearrange, &FftMask, pp, &net, sid), dist-primitives/src/dfft/mod.rs:99-134: share_d [m/l] in place,
 * masks [m/l] or NULL */
int zk_party_d_fft(zk_ctx* ctx, zk_party* p, int sid, void* share_d, const void* in_mask_d, const void* out_mask_d,
                   int rearrange, int log2_m, uint64_t seed, void* stream);
/* d_ifft(pd_shares, rearrange, &FftMask, dom, g, pp, &net, sid), dfft/mod.rs:137-175 */
int zk_party_d_ifft(zk_ctx* ctx, zk_party* p, int sid, void* share_d, const void* in_mask_d, const void* out_mask_d,
                    int rearrange, int log2_m, const void* g, uint64_t seed, void* stream);
/* deg_red(px, pp, &DegRedMask, &net, sid), dist-primitives/src/utils/deg_red.rs:80-126: x_d [len] in place */
int zk_party_deg_red(zk_ctx* ctx, zk_party* p, int sid, void* x_d, const void* in_mask_d, const void* out_mask_d, size_t len,
                     uint64_t seed, void* stream);
/* d_pp(num, den, &DegRedMask, pp, &net, sid), dist-primitives/src/dpp/mod.rs:15-87: num_d, den_d, out_d [len] */
int zk_party_d_pp(zk_ctx* ctx, zk_party* p, int sid, const void* num_d, const void* den_d, const void* in_mask_d,
                  const void* out_mask_d, size_t len, uint64_t seed, void* out_d, void* stream);
/* d_msm(bases, scalars, &MsmMask, pp, &net, sid), dist-primitives/src/dmsm/mod.rs:59-102: bases_d, scalars_d [len];
 * in_mask / out_mask: ONE Jacobian point each (host) or NULL; out: one Jacobian point (host) */
int zk_party_d_msm(zk_ctx* ctx, zk_party* p, int sid, int group, const void* bases_d, const void* scalars_d, size_t len,
                   const void* in_mask, const void* out_mask, void* out, void* stream);
/* circom_h(qap_share, pp, masks.., &net), groth16/src/ext_wit.rs:104-181: qap_*_d, h_d [m/l]; the Fr-vector members of
 * `masks` are THIS PARTY's rows (the MSM members are not read) */
int zk_party_circom_h(zk_ctx* ctx, zk_party* p, const void* qap_a_d, const void* qap_b_d, const void* qap_c_d, int log2_m,
                      const zk_groth16_masks* masks, uint64_t seed, void* h_d, void* stream);
/* dsha256(pp, crs_share, qap_share, a_share, ax_share, .., &net), groth16/examples/sha256.rs:32-129: the five share vectors of
 * `crs` (s_d .. u_d, [len] each), the QAP and witness shares and every member of `masks` are THIS PARTY's rows (MSM masks:
 * one Jacobian point each, host); pi_a / pi_c: one Jacobian G1, pi_b: one Jacobian G2 (host).  The members of `crs` that are
 * not party rows (a_query0, b_g1_query0, delta_g1, alpha_g1, beta_g1, b_g2_query0, delta_g2, beta_g2) are taken from the
 * RANK'S FIRST PARTY; the lengths must agree across the round. */
int zk_party_groth16_prove(zk_ctx* ctx, zk_party* p, const zk_crs_share* crs, const void* qap_a_d, const void* qap_b_d,
                           const void* qap_c_d, const void* a_share_d, const void* ax_share_d, const void* r, const void* s,
                           int log2_m, const zk_groth16_masks* masks, uint64_t seed, void* pi_a, void* pi_b, void* pi_c,
                           void* stream);

/* ---- host-pointer forms of the primitives (the reference's own signatures take and return host vectors: dfft/mod.rs:99,
 * dmsm/mod.rs:59): the call stages its operands through device scratch (H2D, compute, D2H) and returns when the result is
 * in host memory.  zk_d_fft_host: shares [n][m/l] in place, masks host [n][m/l] or NULL, inverse != 0 = d_ifft with the
 * coset element g (Montgomery Fr, host, or NULL).  zk_msm_host / zk_d_msm_host: affine bases and scalars in host memory,
 * results as zk_msm / zk_d_msm.  The device-pointer forms stay the fast path: a 2^20 d_fft moves 2 x 128 MiB over PCIe
 * (~4.3 ms at 63 GB/s) around 0.87 ms of compute. */
int zk_d_fft_host(zk_ctx* ctx, void* shares, const void* in_mask, const void* out_mask, int rearrange, int log2_m,
                  int inverse, const void* g, uint64_t seed, void* stream);
/* The same staging for the remaining functions whose reference signatures take host vectors (round 4):
 * zk_deg_red_host      dist-primitives/src/utils/deg_red.rs:80 (px: Vec<T>): x [n][len] in place, masks host [n][len] or NULL
 * zk_d_pp_host         dist-primitives/src/dpp/mod.rs:15 (num, den: Vec<F>): out [n][len] host
 * zk_circom_h_host     groth16/src/ext_wit.rs:104 (PackedQAPShare of Vec<F>): qap_* and h host [n][m/l]; the Fr-vector members
 *                      of `masks` (fft_in / fft_out / degred_*) are HOST pointers here
 * zk_groth16_prove_host  groth16/examples/sha256.rs:32 (dsha256 over host vectors): the five share vectors of `crs`, the QAP and
 *                      witness shares and the Fr-vector masks are HOST pointers; the single CRS elements, r, s and the MsmMasks are
 *                      host values as in zk_groth16_prove.  PCIe-inclusive: never what bench.py times. */
int zk_deg_red_host(zk_ctx* ctx, void* x, const void* in_mask, const void* out_mask, size_t len, uint64_t seed, void* stream);
int zk_d_pp_host(zk_ctx* ctx, const void* num, const void* den, const void* in_mask, const void* out_mask, size_t len,
                 uint64_t seed, void* out, void* stream);
int zk_circom_h_host(zk_ctx* ctx, const void* qap_a, const void* qap_b, const void* qap_c, int log2_m,
                     const zk_groth16_masks* masks, uint64_t seed, void* h, void* stream);
int zk_groth16_prove_host(zk_ctx* ctx, const zk_crs_share* crs, const void* qap_a, const void* qap_b, const void* qap_c,
                          const void* a_share, const void* ax_share, const void* r, const void* s, int log2_m,
                          const zk_groth16_masks* masks, uint64_t seed, void* pi_a, void* pi_b, void* pi_c, void* stream);
int zk_msm_host(zk_ctx* ctx, int group, const void* bases, size_t len_bases, const void* scalars, size_t len_scalars,
                void* out, void* stream);
int zk_d_msm_host(zk_ctx* ctx, int group, const void* bases, const void* scalars, size_t len, const void* in_mask,
                  const void* out_mask, void* out, void* stream);

/* ---- per-kernel timing (measurement only) -----------------------------------------------------------------
 * When enabled, HIP events are recorded on the launching stream around the kernels of each slot; zk_profile_read
 * synchronises them and returns the summed duration, the summed work units (elements / chunks / points) and the
 * number of timed launches since zk_profile_enable.  Slots whose name starts with "host:" are host spans of
 * zk_groth16_prove taken with the steady clock instead (entry -> everything launched -> the event of the last chain ->
 * return; units = calls). */
int zk_profile_enable(zk_ctx* ctx, int on);
/* MSM work counters of this context since creation (measurement only): stats[0] / [1] = mixed additions the G1 / G2
 * accumulate kernels performed (= sorted (point, window) entries: identity bases and zero digits leave none), stats[2] /
 * [3] = (point, window) pairs offered to the sorts.  Counted when an MSM's result is collected. */
int zk_msm_stats(zk_ctx* ctx, uint64_t stats[4]);
int zk_profile_slots(void);
const char* zk_profile_name(int slot);
int zk_profile_read(zk_ctx* ctx, int slot, double* total_ms, double* units, long* calls);

/* d_msm when some parties dropped out: bases_d / scalars_d / in_mask hold the `nparties` surviving parties (ascending
 * ids); out (n Jacobian points) as zk_d_msm. */
int zk_d_msm_parties(zk_ctx* ctx, int group, const void* bases_d, const void* scalars_d, size_t len,
                     const uint32_t* parties, int nparties, const void* in_mask, const void* out_mask, void* out,
                     void* stream);

/* ---- the verifier: pairings and Groth16 verification on the device (BN254 and BLS12-381) --------------------
 * A BLS12-377 context returns ZK_ERR_BAD_INPUT ("no pairing parameters") from every function of this section.
 *
 * zk_multi_pairing = ark-ec Pairing::multi_pairing: out[i] = final_exp(prod_j miller(P[i][j], Q[i][j])), i < count, j < k.
 * p_affine_d [count][k] G1 affine, q_affine_d [count][k] G2 affine, gt_out_d [count][12] Fq (Montgomery), coefficient
 * order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... = arkworks' Fp12 in memory = snarkjs' [2][3][2] nesting.  An identity in
 * either slot of a pair contributes 1.  Points are taken as given (no curve or subgroup check; zk_points_subgroup_check
 * tests a vector of points, and off the subgroups the pairing is not bilinear).  The BN254 final
 * exponentiation raises to the exponent of the Fuentes-Castaneda chain that arkworks and snarkjs use, so the values are
 * theirs; BLS12-381 uses the exact (q^12 - 1) / r.  Returns when the result is in gt_out_d. */
int zk_multi_pairing(zk_ctx* ctx, const void* p_affine_d, const void* q_affine_d, size_t k, size_t count, void* gt_out_d,
                     void* stream);
/* Parity access to the lane-split Fq12 tower the pairing kernels run on (like zk_fq_selftest): a_d, b_d, out_d [len][12]
 * Fq in the order above; op 0 mul, 1 sqr, 2 inverse, 3 conjugate, 4 / 5 / 6 Frobenius^1..3, 7 cyclotomic squaring (a in
 * the cyclotomic subgroup), 8 a * (l0 + lS w^S + l3 w^3) with l0, lS, l3 = the first three Fq2 of b (the line of a Miller
 * step; S = 1 on BN254's D-type twist, 2 on BLS12-381's M-type twist).  b_d may be NULL for ops 1..7. */
int zk_fq12_selftest(zk_ctx* ctx, int op, const void* a_d, const void* b_d, size_t len, void* out_d, void* stream);
/* ark_groth16 prepare_verifying_key / verify_proof (groth16/examples/sha256.rs:400-415).
 * zk_groth16_vk_prepare: host affine points (gamma_abc_g1: n_abc of them); e(alpha, beta) is computed here, once.
 * zk_groth16_verify: proofs_affine = [count][8 |Fq| limbs], exactly what zk_groth16_reconstruct writes (A | B | C), host;
 * public_inputs = [count][n_inputs] Fr in Montgomery form, host, WITHOUT the leading 1; n_inputs + 1 != n_abc returns
 * ZK_ERR_BAD_INPUT ("malformed verifying key").  Per proof: acc = abc[0] + sum_i x_i abc[i + 1];
 * ok[i] = (final_exp(miller(A, B) miller(acc, -gamma) miller(C, -delta)) == e(alpha, beta)).  A point of a proof that is
 * not on its curve (or a coordinate that is not below q) gives ok[i] = 0, not an error.  As in verify_proof there is NO
 * G2 subgroup check (nor a G1 one): a caller whose proofs come from outside calls zk_groth16_verify_bytes on their wire
 * bytes, or zk_points_subgroup_check on the points, instead.  Every step runs on the
 * device; the call returns with ok filled, and its wait honours the option wait_deadline_ms. */
typedef struct zk_vk zk_vk;
int zk_groth16_vk_prepare(zk_ctx* ctx, const void* alpha_g1, const void* beta_g2, const void* gamma_g2,
                          const void* delta_g2, const void* gamma_abc_g1, size_t n_abc, zk_vk** out);
void zk_groth16_vk_free(zk_vk* vk);
int zk_groth16_verify(zk_ctx* ctx, const zk_vk* vk, const void* proofs_affine, const void* public_inputs, size_t n_inputs,
                      size_t count, uint8_t* ok, void* stream);
/* One verdict for a whole batch: "are all of these good?" by ONE randomized pairing check (count + 3 Miller loops and one
 * final exponentiation, where zk_groth16_verify pays three and one per proof).  vk, proofs_affine, public_inputs, n_inputs,
 * count, stream and the argument errors are those of zk_groth16_verify.  With r_i = the 128-bit randomizers below,
 * s = sum r_i, s_t = sum_i r_i x_{i,t} (mod r), P_gamma = s abc[0] + sum_t s_t abc[t + 1], P_delta = sum_i r_i C_i:
 *   *all_ok = 1 iff every proof passes the curve test of zk_groth16_verify (canonical coordinates, A, B, C on their curves)
 *   AND prod_i e(r_i A_i, B_i) e(P_gamma, -gamma) e(P_delta, -delta) e(-s alpha, beta) = 1.
 * count = 0 gives *all_ok = 1 and launches nothing.  gt_out (host, [12] Fq in Montgomery form, the coefficient order of
 * zk_multi_pairing; may be NULL) receives the value of that product after the final exponentiation -- parity access like
 * zk_fq12_selftest: 1 for an accepted batch, the oracle's multi_pairing of the count + 3 pairs otherwise.
 * seed = 32 bytes that whoever produced the proofs cannot predict, fresh for every call; NULL = the library draws them
 * from the operating system's generator (the source that keys a context's ChaCha stream).  r_i = w0 | w1 << 32 | w2 << 64 |
 * w3 << 96 with w = zk_chacha20_block(key = the seed as eight little-endian words, counter = i, nonce = 0x5A4B524C43); a
 * zero draw is replaced by 1.
 * GUARANTEE AND ITS LIMIT.  For proofs whose points lie in the order-r subgroups the verdict equals "every ok[i] of
 * zk_groth16_verify is 1", except with probability at most 2^-128 over the seed (a batch with a bad proof is accepted
 * only when the randomizers hit one residue mod r).  As in zk_groth16_verify there is NO subgroup check: outside the
 * subgroups (possible for G2 on both curves and for G1 on BLS12-381) bilinearity does not hold and the two calls may
 * disagree; a caller whose proofs come from outside calls zk_groth16_verify_all_bytes, which makes the check, instead.
 * After a 0, zk_groth16_verify on the same
 * arrays says which proofs failed.  WHEN TO USE WHICH (measured on one MI355X): the batch call is the
 * faster one from 4096 proofs on BN254 and from 16384 on BLS12-381 (2.8x / 3.2x at 65536); below 4096 it is 3-8 ms slower
 * than zk_groth16_verify, which also names the bad proof.
 * Every step runs on the device; the call returns with the verdict on the host, and its wait honours wait_deadline_ms. */
int zk_groth16_verify_all(zk_ctx* ctx, const zk_vk* vk, const void* proofs_affine, const void* public_inputs,
                          size_t n_inputs, size_t count, const uint8_t* seed, int* all_ok, void* gt_out, void* stream);

/* ---- subgroup membership, and verification from wire bytes (BN254 and BLS12-381; BLS12-377: ZK_ERR_BAD_INPUT) ----------
 * zk_points_subgroup_check = ark-ec's is_in_correct_subgroup_assuming_on_curve after the curve test, on a device vector of
 * affine Montgomery points [len]: ok_d[i] (device, one byte) = 1 iff both coordinates are below q and the point is the
 * identity (0, 0) or lies on its curve with [r]P = O.  A point off its curve gives 0 and is never an error; len = 0 launches
 * nothing.  The tests are those of ark-bn254 / ark-bls12-381 0.4: BN254 G1 has cofactor 1 (the curve equation decides);
 * BN254 G2 psi(P) = [6x^2]P in the form of eprint 2022/352 4.3 that multiplies by x only; BLS12-381 G2 psi(P) = [x]P;
 * BLS12-381 G1 phi(P) = -[x^2]P.  Fixed chains of 63 / 64 doublings: no loop bound depends on the point.
 * Returns when ok_d is written. */
int zk_points_subgroup_check(zk_ctx* ctx, int group, const void* affine_d, size_t len, uint8_t* ok_d, void* stream);
/* zk_groth16_reconstruct_robust: a batch of proofs from proof shares that are NOT trusted.  zk_groth16_reconstruct trusts
 * every share: one wrong share gives a proof that fails verification, and nobody is named.  Here r and s are in the clear
 * (oracle/groth16.py dist_prove), so a party's shares of A, B and C are fixed linear combinations of d_msm outputs and clear
 * points: each of the three is a word of DIMENSION 2l, not 4l - 1.  With nparties listed that leaves nparties - 2l
 * syndromes: one wrong share per element is located and corrected when nparties >= 2l + 2 (up to 2l - 2 parties may be
 * absent at the same time); nparties == 2l + 1 detects only.
 * pi_a / pi_c: [nproofs][nparties] Jacobian G1, pi_b: [nproofs][nparties] Jacobian G2, HOST, column i the share of parties[i]
 * (ascending ids, NULL = 0 .. nparties - 1) -- with all parties, what zk_groth16_prove_batch / zk_groth16_batch_wait write.
 * The shares are copied up once; per element one staging kernel writes the compact affine [nparties][nproofs] (Z == 0 is the
 * identity), every staged share is tested with the predicate of zk_points_subgroup_check (on the curve and [r]P = O), and
 * A SHARE THAT FAILS THE PREDICATE IS REPLACED BY THE IDENTITY BEFORE DECODING: from there on it is an ordinary wrong share,
 * located, corrected and named in errpos like any other.  Then zk_pss_unpack_points_robust_parties runs at dimension 2l, once
 * for A (G1), B (G2) and C (G1), chunk = proof; secret 0 of a chunk is the element.
 *   status (host, [nproofs][3])            0, 1 or 2 for A, B, C of proof i, as that call's
 *   errpos (host, [nproofs][3], or NULL)   bit p: party p's share of that element was corrected
 *   proofs_affine (host, or NULL)          [nproofs] A | B | C as zk_groth16_reconstruct writes them; a failed element is (0, 0)
 *   proofs_bytes (host, or NULL)           [nproofs][4 |Fq|] as zk_groth16_reconstruct's, through the same device codec; the
 *                                          bytes of a proof with ANY failed element are all zero
 * A failed element is not an error return.  Errors: the list refusals of zk_pss_unpack_points_robust_parties, then NULL status
 * -> ZK_ERR_BAD_INPUT, then nparties <= 2l -> ZK_ERR_PROTOCOL; nproofs == 0 is then ZK_OK and nothing is written, whatever the
 * other pointers are; NULL pi_a / pi_b / pi_c with nproofs > 0, or more than 2^32 / n proofs -> ZK_ERR_BAD_INPUT.  A context
 * without G2 or without subgroup parameters (BLS12-377) -> ZK_ERR_BAD_INPUT.  Synchronous, like zk_groth16_reconstruct; the
 * working memory is the context's own (one call at a time per context).  Device engine only. */
int zk_groth16_reconstruct_robust(zk_ctx* ctx, size_t nproofs, const void* pi_a, const void* pi_b, const void* pi_c,
                                  const uint32_t* parties, int nparties, void* proofs_affine /* host, or NULL */,
                                  void* proofs_bytes /* host, or NULL */, uint8_t* status /* host [nproofs][3] */,
                                  uint32_t* errpos /* host [nproofs][3], or NULL */, void* stream);
/* CanonicalDeserialize::deserialize_compressed with validation (Validate::Yes), per element: decodes exactly as
 * zk_points_decompress does (both encodings, the same flag rules) and tests the subgroup.  A bad element does not fail
 * the call: ok_d[i] = 0 and (0, 0) is written for an encoding that does not decode; ok_d[i] = 0 and the decoded point is
 * kept for a point outside the order-r subgroup; ok_d[i] = 1 otherwise. */
int zk_points_decompress_checked(zk_ctx* ctx, int group, const void* bytes_d, size_t len, void* out_affine_d, uint8_t* ok_d,
                                 void* stream);
/* Groth16::verify_proof after Proof::deserialize_compressed (with validation) and Fr::deserialize_compressed of the
 * public inputs, all on the device: what a verifier that takes proofs from strangers calls.
 * proof_bytes (host) = [count][4 |Fq| bytes], exactly what zk_groth16_reconstruct writes as proof_bytes (128 bytes on
 * BN254, 192 on BLS12-381 in the zcash form); input_bytes (host) = [count][n_inputs][32], little-endian canonical Fr,
 * WITHOUT the leading 1.  ok[i] = 1 iff A, B and C decode, lie in their order-r subgroups, every input is below r and the
 * pairing equation of zk_groth16_verify holds.  A defect of any kind gives ok[i] = 0 for that proof only, never an error;
 * the argument errors are those of zk_groth16_verify.  The bytes are copied up once; two launches decode them into the
 * arrays zk_groth16_verify stages, whose verdict kernels then run unchanged. */
int zk_groth16_verify_bytes(zk_ctx* ctx, const zk_vk* vk, const void* proof_bytes, const void* input_bytes, size_t n_inputs,
                            size_t count, uint8_t* ok, void* stream);
/* The one randomized verdict of zk_groth16_verify_all from the same bytes: seed, all_ok and gt_out as there.  *all_ok = 0
 * as soon as any proof fails decoding, the subgroup test or the input range; with every point in its subgroup the
 * guarantee of zk_groth16_verify_all holds without its limit. */
int zk_groth16_verify_all_bytes(zk_ctx* ctx, const zk_vk* vk, const void* proof_bytes, const void* input_bytes,
                                size_t n_inputs, size_t count, const uint8_t* seed, int* all_ok, void* gt_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZKSAAS_H */
