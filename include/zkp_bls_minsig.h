/*
 * include/zkp_bls_minsig.h -- the minimal-signature-size BLS layer of libzkp_pairings.so: messages hashed to points of G1 on the GPU and
 * two batch verifiers on top of them.  A tenth header of the SAME library: include it beside zkp_bls.h, whose message layout (one byte
 * buffer plus n + 1 offsets), DST argument and limits, rand (2 u64 per signature), ZKP_BLS_POINTS_CHECKED and validation word it shares,
 * and zkp_pairings.h (zkp_ctx, zkp_status codes, wire formats: 6 u64 per Fp, G1 = 12 u64, G2 = 24 u64, infinity bytes, the identity
 * written as (0, 1)).  Symbols added under ABI version 4 (zkp_abi_version() is still 4).  This is where the follow-up that zkp_bls.h
 * names as out of scope went.
 *
 * The suite is RFC 9380 BLS12381G1_XMD:SHA-256_SSWU_RO_; the scheme is minimal-signature-size: signatures in G1, public keys in G2 -
 * the layout of drand's quicknet beacons, whose DST is "BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_" (43 bytes), of the
 * BLS_SIG_BLS12381G1_* suites of the BLS draft; the map is the one behind EIP-2537's MAP_FP_TO_G1 (that precompile maps ONE field
 * element; zkp_g1_map_from_fields_batch sums the images of two).
 *
 * Every entry point has a host-pointer flavour and a _dev flavour with a trailing stream, under the contract of zkp_bls.h: the _dev
 * flavour is asynchronous, reads nothing back, and is capturable into a hipGraph once the context's workspaces have reached the call's
 * size (run the call once before capturing it).  Messages and offsets follow zkp_bls.h to the letter: a message whose offsets decrease,
 * or leave [offsets[0], offsets[n]], is hashed as the EMPTY message and in validation mode ORs into the validation word; the host
 * flavour refuses such offsets with ZKP_ERR_ARG.
 *
 * zkp_hash_to_field_g1_batch    out_u: n x 2 Fp (u0, u1: 12 u64 per message) - expand_message_xmd to 128 bytes (L = 64, count = 2, m = 1),
 *                               two reductions
 * zkp_g1_map_from_fields_batch  u (n x 2 Fp, canonical) -> clear_cofactor(iso(sswu(u0)) + iso(sswu(u1)))
 * zkp_g1_clear_cofactor_batch   points of E - any points of the curve y^2 = x^3 + 4, not only of G1 - to [1 - x] P = [0xd201000000010001] P
 * zkp_hash_to_g1_batch          the composition; the u values never leave the device
 * zkp_bls_minsig_verify_batch   *all_ok = ( prod_i e([r_i] H(m_i), pk_i) * e(sum_i [r_i] sig_i, -g2) == 1 ) with r_i = a_i + b_i z^2 from
 *                               rand, as zkp_bls_verify_batch: the hashed points go to the driver of zkp_pairing_check_batch_rlc as one
 *                               free pair (H(m_i), pk_i) per check and one s2 column (sig_i, -g2) - a G1 MSM, the Groth16 shape; there
 *                               is no second pairing path.  Unless flags has ZKP_BLS_POINTS_CHECKED, pk and sig go through is_valid
 *                               first; H(m_i) needs no check.  An identity among the public keys (KeyValidate), an invalid point, a zero
 *                               (a_i, b_i) give all_ok = 0, not an error.  n == 0 gives 1.
 * zkp_bls_minsig_verify_samekey_batch   ONE key (pk: one G2 point, 24 u64) signed every message: the driver with k = 0 and s2 = 2,
 *                               columns (H(m_i), pk) and (sig_i, -g2) - two G1 MSMs, two Miller loops, one final exponentiation.  Its
 *                               answer is that of zkp_bls_minsig_verify_batch with the key repeated n times and the same rand.  The
 *                               identity as the wire writes it, (0, 1), and a key outside G2 give 0.
 * ZKP_ERR_ARG, before a byte is read: dst_len == 0 or dst_len > 255; n beyond 2^31 - 1, for the verifiers beyond 2^24 (the batch check's
 * limit with a column); null pointers with non-zero counts (inf_pk, inf_sig and the inf of zkp_g1_clear_cofactor_batch may be null: no
 * infinities; the same-key verifier's pk is required even for n == 0); unknown flags.  Validation mode covers u, the points, pk and sig.
 *
 * How (zkvm_pairings_amd/csrc/zkp_bls_minsig.hip, zkp_h2f.hpp, zkp_bls_minsig_plan.hpp): k_g1h_field, a lane per message, the SHA-256 and
 * reduction code of k_h2f with four output blocks; k_g1h_map, a lane per field element: the straight-line simplified SWU on E1' (Z = 11)
 * with ONE fixed exponentiation (sqrt_ratio for p = 3 mod 4: root, branch and division together, x stays a fraction), the sign, the
 * 11-isogeny on the fraction by homogenised Horner steps to a projective point of E (a pole of the isogeny is the identity);
 * k_g1h_clear, a lane per point: the sum and a 64-bit double-and-add with the complete addition formulas of Renes, Costello and Batina;
 * k_g1h_affine: one inversion per wavefront of 64.  The isogeny's coefficients are derived by tools/gen_constants.py (Velu's formulas on
 * the rational subgroup of order 11, then the one scaling of six that reproduces the RFC's vectors).
 * Cost: per message 4 + ceil((len + dst_len + 13) / 64) + 4 ceil((dst_len + 43) / 64) SHA-256 blocks, two exponentiations of 461
 * products (one per u), about 150 products of isogeny, about 1250 of group law and 1 / 64 of an inversion - unmeasured.
 * Slices and workspace (grow-only, owned by the context, separate from zkp_bls.h's): slices of 2^17 messages; per message of a slice
 * 96 B of u, 336 B of mapped points and 168 B of cleared sums, plus for the verifiers 99 B per signature (the hashed point, its infinity
 * byte, two status bytes; 196 B for the same-key verifier, whose rows hold the signature too) and the workspaces of
 * zkp_pairing_check_batch_rlc with k = 1, s2 = 1 (k = 0, s2 = 2).
 *
 * Out of scope: the _NU_ (encode-to-curve) suites, DSTs over 255 bytes, grouping by message for this layout, more than one GPU.
 * Committee aggregation for G2 keys (a G2 segment sum) went to zkp_bls_agg_g2.h.
 */
#ifndef ZKP_BLS_MINSIG_H
#define ZKP_BLS_MINSIG_H

#include "zkp_bls.h"

#ifdef __cplusplus
extern "C" {
#endif

int zkp_hash_to_field_g1_batch(zkp_ctx* ctx, const uint8_t* msgs, const uint64_t* offsets /* n + 1 */, size_t n, const uint8_t* dst, size_t dst_len,
                               uint64_t* out_u /* n x 12 */);
int zkp_hash_to_field_g1_batch_dev(zkp_ctx* ctx, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len, void* d_out_u,
                                   void* stream);
int zkp_g1_map_from_fields_batch(zkp_ctx* ctx, const uint64_t* u /* n x 12 */, size_t n, uint64_t* out /* n x 12 */, uint8_t* out_inf /* n */);
int zkp_g1_map_from_fields_batch_dev(zkp_ctx* ctx, const void* d_u, size_t n, void* d_out, void* d_out_inf, void* stream);
int zkp_g1_clear_cofactor_batch(zkp_ctx* ctx, const uint64_t* pts /* n x 12 */, const uint8_t* inf, size_t n, uint64_t* out, uint8_t* out_inf);
int zkp_g1_clear_cofactor_batch_dev(zkp_ctx* ctx, const void* d_pts, const void* d_inf, size_t n, void* d_out, void* d_out_inf, void* stream);
int zkp_hash_to_g1_batch(zkp_ctx* ctx, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len, uint64_t* out,
                         uint8_t* out_inf);
int zkp_hash_to_g1_batch_dev(zkp_ctx* ctx, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len, void* d_out,
                             void* d_out_inf, void* stream);
int zkp_bls_minsig_verify_batch(zkp_ctx* ctx, const uint64_t* pk /* n x 24 */, const uint8_t* inf_pk, const uint8_t* msgs, const uint64_t* offsets,
                                const uint8_t* dst, size_t dst_len, const uint64_t* sig /* n x 12 */, const uint8_t* inf_sig, size_t n,
                                const uint64_t* rand /* n x 2 */, int flags, int* all_ok);
int zkp_bls_minsig_verify_batch_dev(zkp_ctx* ctx, const void* d_pk, const void* d_inf_pk, const void* d_msgs, const void* d_offsets, const void* d_dst,
                                    size_t dst_len, const void* d_sig, const void* d_inf_sig, size_t n, const void* d_rand, int flags, void* d_all_ok,
                                    void* stream);
int zkp_bls_minsig_verify_samekey_batch(zkp_ctx* ctx, const uint64_t* pk /* 24 */, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst,
                                        size_t dst_len, const uint64_t* sig /* n x 12 */, const uint8_t* inf_sig, size_t n,
                                        const uint64_t* rand /* n x 2 */, int flags, int* all_ok);
int zkp_bls_minsig_verify_samekey_batch_dev(zkp_ctx* ctx, const void* d_pk, const void* d_msgs, const void* d_offsets, const void* d_dst, size_t dst_len,
                                            const void* d_sig, const void* d_inf_sig, size_t n, const void* d_rand, int flags, void* d_all_ok,
                                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
