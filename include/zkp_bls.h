/*
 * include/zkp_bls.h -- the BLS signature layer of libzkp_pairings.so: messages hashed to points of G2 on the GPU and a batch verifier on top
 * of them.  A seventh header of the SAME library: include it beside zkp_pairings.h, whose zkp_ctx, zkp_status codes, wire formats (6 u64
 * per Fp, G1 = 12 u64, G2 = 24 u64, infinity bytes, the identity written as (0, 1)), zkp_set_validate and validation word
 * (zkp_take_validation_status_dev) it shares.  Symbols added under ABI version 4 (zkp_abi_version() is still 4).
 *
 * The suite is RFC 9380 BLS12381G2_XMD:SHA-256_SSWU_RO_; the scheme is minimal-pubkey-size: public keys in G1, signatures in G2.  The
 * domain-separation tag (DST) is an argument of every call; Ethereum's is "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_" (43 bytes).
 *
 * Every entry point has a host-pointer flavour and a _dev flavour with a trailing stream.  The _dev flavour is asynchronous, reads nothing
 * back, and is capturable into a hipGraph once the context's workspaces have reached the call's size (run the call once before capturing
 * it) - the contract of zkp_pairing_check_batch_rlc_dev.
 *
 * Messages: ONE byte buffer plus offsets, n + 1 u64 values, non-decreasing; message i is msgs[offsets[i] .. offsets[i + 1]).  Empty
 * messages are legal.  For the _dev flavour the offsets (and the DST) live on the device and the host never reads them.  A message whose
 * offsets decrease, or leave [offsets[0], offsets[n]], never makes a kernel read outside that range: it is hashed as the EMPTY message, and
 * in validation mode it ORs into the validation word.  The host flavour, which sees the offsets, refuses them with ZKP_ERR_ARG.
 *
 * zkp_fp_from_wide_be_batch     64 big-endian bytes per element -> canonical Fp, OS2IP(bytes) mod p: the reduction of hash_to_field on
 *                               chosen operands
 * zkp_hash_to_field_g2_batch    out_u: n x 2 Fp2 (u0, u1: 24 u64 per message) - expand_message_xmd to 256 bytes (L = 64, count = 2, m = 2),
 *                               four reductions
 * zkp_g2_map_from_fields_batch  u (n x 2 Fp2, canonical) -> clear_cofactor(iso(sswu(u0)) + iso(sswu(u1)))
 * zkp_g2_clear_cofactor_batch   points of E2 - any points of the curve y^2 = x^3 + 4 (1 + i), not only of G2 - to [h_eff] P, computed as
 *                               [x^2 - x - 1] P + [x - 1] psi(P) + psi^2(2 P) with x = -0xd201000000010000
 * zkp_hash_to_g2_batch          the composition; the u values never leave the device
 * zkp_bls_verify_batch          *all_ok = ( prod_i e([r_i] pk_i, H(m_i)) * e(-g1, sum_i [r_i] sig_i) == 1 ) with r_i = a_i + b_i z^2 from
 *                               rand (2 u64 per signature, as zkp_pairing_check_batch_rlc): the hashed points go to that call's driver as
 *                               one free pair per check and one column with the fixed point -g1; there is no second pairing path.  Unless
 *                               flags has ZKP_BLS_POINTS_CHECKED, pk and sig go through is_valid first; H(m_i) needs no check.  An identity
 *                               among the public keys (KeyValidate), an invalid point, a zero (a_i, b_i) give all_ok = 0, not an error.
 *                               n == 0 gives 1.
 * ZKP_ERR_ARG, before a byte is read: dst_len == 0 or dst_len > 255 (the oversize-DST rule of RFC 9380 5.3.3 is out of scope); n beyond
 * 2^31 - 1, for the verifier beyond 2^24 (the batch check's limit with a column); null pointers with non-zero counts (inf_pk, inf_sig and
 * the inf of zkp_g2_clear_cofactor_batch may be null: no infinities); unknown flags.  Validation mode covers u, the points, pk and sig.
 *
 * How (zkvm_pairings_amd/csrc/zkp_bls.hip, zkp_bls_clear.hip, zkp_bls_plan.hpp): k_h2f, a lane per message, SHA-256 with the schedule in 16 rolling registers
 * and each 64-byte slice reduced from the registers by one two-product Montgomery reduction; k_h2c_map, a lane per field element:
 * simplified SWU on E' (three fixed exponentiations: one inversion, two for the square root, which also decides the branch), the sign, the
 * 3-isogeny to a projective point of E2 (a pole of the isogeny is the identity); k_h2c_clear, two lanes per point: the sum and the
 * cofactor by two 64-bit ladders with complete additions.
 * Cost: per message 4 + ceil((len + dst_len + 13) / 64) + 8 ceil((dst_len + 43) / 64) SHA-256 blocks, six exponentiations of 461
 * products and about 2600 Fp2 products of group law - unmeasured.
 * Slices and workspace (grow-only, owned by the context): slices of 2^17 messages; per message of a slice 192 B of u and 672 B of
 * projective points, plus for the verifier 195 B per signature (the hashed point, its infinity byte, two status bytes) and the workspaces
 * of zkp_pairing_check_batch_rlc with k = 1, s1 = 1.
 *
 * Out of scope: hashing to G1 (the minimal-signature-size variants: they are include/zkp_bls_minsig.h), DSTs over 255 bytes, ragged
 * per-signature committees (they are include/zkp_bls_agg.h), proof-of-possession management, more than one GPU.
 */
#ifndef ZKP_BLS_H
#define ZKP_BLS_H

#include "zkp_pairings.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKP_BLS_POINTS_CHECKED 1   /* flags: skip is_valid on pk and sig (the caller guarantees them) */

int zkp_fp_from_wide_be_batch(zkp_ctx* ctx, const uint8_t* bytes /* n x 64 */, size_t n, uint64_t* out /* n x 6 */);
int zkp_fp_from_wide_be_batch_dev(zkp_ctx* ctx, const void* d_bytes, size_t n, void* d_out, void* stream);
int zkp_hash_to_field_g2_batch(zkp_ctx* ctx, const uint8_t* msgs, const uint64_t* offsets /* n + 1 */, size_t n, const uint8_t* dst, size_t dst_len,
                               uint64_t* out_u /* n x 24 */);
int zkp_hash_to_field_g2_batch_dev(zkp_ctx* ctx, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len, void* d_out_u,
                                   void* stream);
int zkp_g2_map_from_fields_batch(zkp_ctx* ctx, const uint64_t* u /* n x 24 */, size_t n, uint64_t* out /* n x 24 */, uint8_t* out_inf /* n */);
int zkp_g2_map_from_fields_batch_dev(zkp_ctx* ctx, const void* d_u, size_t n, void* d_out, void* d_out_inf, void* stream);
int zkp_g2_clear_cofactor_batch(zkp_ctx* ctx, const uint64_t* pts /* n x 24 */, const uint8_t* inf, size_t n, uint64_t* out, uint8_t* out_inf);
int zkp_g2_clear_cofactor_batch_dev(zkp_ctx* ctx, const void* d_pts, const void* d_inf, size_t n, void* d_out, void* d_out_inf, void* stream);
int zkp_hash_to_g2_batch(zkp_ctx* ctx, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len, uint64_t* out,
                         uint8_t* out_inf);
int zkp_hash_to_g2_batch_dev(zkp_ctx* ctx, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len, void* d_out,
                             void* d_out_inf, void* stream);
int zkp_bls_verify_batch(zkp_ctx* ctx, const uint64_t* pk /* n x 12 */, const uint8_t* inf_pk, const uint8_t* msgs, const uint64_t* offsets,
                         const uint8_t* dst, size_t dst_len, const uint64_t* sig /* n x 24 */, const uint8_t* inf_sig, size_t n,
                         const uint64_t* rand /* n x 2 */, int flags, int* all_ok);
int zkp_bls_verify_batch_dev(zkp_ctx* ctx, const void* d_pk, const void* d_inf_pk, const void* d_msgs, const void* d_offsets, const void* d_dst,
                             size_t dst_len, const void* d_sig, const void* d_inf_sig, size_t n, const void* d_rand, int flags, void* d_all_ok,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
