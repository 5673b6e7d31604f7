/*
 * include/zkp_bls_grouped.h -- BLS batch verification GROUPED BY MESSAGE of libzkp_pairings.so: n signatures over m distinct messages
 * verified with m hashes to G2 and m + 1 Miller loops instead of n and n + 1, and the sum of scaled G1 points per segment that makes it
 * possible.  A ninth header of the SAME library: include it beside zkp_bls_agg.h, whose committee arguments (table, idx, seg_off) the
 * aggregate form shares, zkp_bls.h (the message layout: one byte buffer plus count + 1 offsets, the DST argument, rand (2 u64 per
 * signature), ZKP_BLS_POINTS_CHECKED) and zkp_pairings.h (zkp_ctx, status codes, wire formats: G1 = 12 u64, G2 = 24 u64, infinity bytes,
 * the identity written as (0, 1), zkp_set_validate and the validation word).  Symbols added under ABI version 4 (zkp_abi_version() is
 * still 4).  This is where the follow-up that zkp_bls_agg.h names as out of scope went.
 *
 * Every entry point has a host-pointer flavour and a _dev flavour with a trailing stream.  The _dev flavour is asynchronous, reads nothing
 * back, and is capturable into a hipGraph once the context's workspaces have reached the call's size (run the call once before capturing
 * it) - the contract of zkp_bls_verify_batch_dev.
 *
 * Groups: the n signatures arrive ORDERED BY MESSAGE (the caller sorts; Python: group_by_message), with m + 1 offsets grp_off (u64):
 * signatures grp_off[g] .. grp_off[g + 1] sign message g.  The offsets are well formed when they are non-decreasing from grp_off[0] = 0
 * to grp_off[m] = n.  msgs and offsets (m + 1 values) describe the m DISTINCT messages exactly as in zkp_bls.h.  By bilinearity
 *
 *     prod_i e([r_i] pk_i, H(m_g(i)))  =  prod_g e( sum_{i in group g} [r_i] pk_i , H(m_g) ),     r_i = a_i + b_i z^2
 *
 * zkp_g1_scaled_segment_sum_batch              out[g] = sum over segment g of [a_i + b_i z^2] P_i with (a_i, b_i) = rand[2 i], rand[2 i + 1]:
 *                                              the affine wire point, canonical, so bit-exact whatever the order of addition; the
 *                                              identity is (0, 1) with out_inf = 1.  An empty segment, an input at infinity (inf may be
 *                                              null) and a zero (a_i, b_i) give the identity and are no error; P and -P under one (a, b)
 *                                              cancel; status is 0 unless the call is malformed.  For a point of the curve outside
 *                                              G1 the summand is [a_i] P_i + [b_i] (beta x_i, -y_i), as in zkp_g1_mul_endo_batch.
 * zkp_bls_verify_grouped_batch                 *all_ok = what zkp_bls_verify_batch returns on the same signatures with message g repeated
 *                                              for each member of group g and the same rand: the two products are equal in Gt, so this
 *                                              holds for every input, forged ones included.  The same flag rules: is_valid on pk and sig
 *                                              unless flags has ZKP_BLS_POINTS_CHECKED; an identity public key (inf_pk), an invalid point
 *                                              or a zero (a_i, b_i) give 0, not an error.  A message with no signature is legal and
 *                                              contributes nothing.  n == 0 gives 1, whatever m is.
 * zkp_bls_fast_aggregate_verify_grouped_batch  the committee arguments of zkp_bls_fast_aggregate_verify_batch in place of pk: the
 *                                              segment sums of zkp_g1_segment_sum_batch into the workspace, then the driver above.  An
 *                                              empty committee, a non-zero status and an aggregate that is the identity give 0.
 *
 * Bad input, _dev flavour (the host sees nothing): malformed seg_off / grp_off make the whole call malformed: every sum comes out as the
 * identity with status = 1 (the verifiers: all_ok = 0), the offsets are not followed, nothing outside the arrays is read, and in
 * validation mode the validation word is ORed - the stance of zkp_g1_segment_sum_batch_dev.  The host flavour, which sees the offsets,
 * refuses them with ZKP_ERR_ARG before a byte is copied.
 * ZKP_ERR_ARG in both flavours: null pointers with non-zero counts (seg_off / grp_off count n_seg + 1 / m + 1 values and may be null only
 * when both counts are zero - the verifiers': when n = 0); n > 2^24; n_seg or m > 2^24; m > 0 with null offsets (msgs may be null: every
 * message may be empty); everything zkp_bls_verify_batch and zkp_bls_fast_aggregate_verify_batch refuse.  Validation mode covers the
 * points, the table and the signatures.
 *
 * How (zkvm_pairings_amd/csrc/zkp_bls_grouped.hip, zkp_bls_grouped_plan.hpp): k_grp_zero fills the call's word and the sums; k_grp_check
 * tests the offsets; k_grp_keys, a lane per signature, finds the signature's group by a bounded binary search and writes it as the sort key
 * with the "real contribution" flag of the bucket MSM's partial sums; k_grp_scale (a lane per signature, the joint double-and-add of
 * zkp_g1_mul_endo_batch over the 64 bit pairs of (a, b) with the table P, phi'(P), P + phi'(P) in LDS) stores [r_i] pk_i as a JACOBIAN
 * record - no inversion, no wire point; the bucket MSM's accumulation kernel (k_msm_accum on Jacobian records: 32 sorted records per lane,
 * full additions with every exceptional case of the group law, partial sums joined level by level) sums them - the keys are sorted by
 * construction, there is no sort -; k_grp_affine turns the sums into affine points with ONE inversion per wavefront of 64 sums.  The
 * verifier then hashes the m messages, runs one Miller product over the m pairs (A_g, H_g), one G2 MSM S = sum [r_i] sig_i, one Miller
 * loop on (-g1, S), one final exponentiation of the two values, and ANDs the flags: no second pairing path, no second scaling.
 * Cost: per signature one scaling of about 1,040 Fp products (the 461 of the per-signature inversion are gone), one full addition (16)
 * and a 25-step search; per partial sum of a level a full addition; per group 18 products, 1/64 of an inversion of 461, one hash to G2 and
 * one Miller loop; per call one G2 MSM of n terms, one more Miller loop and one final exponentiation.  Measurements: DESIGN 3.13.
 * Slices and workspace (grow-only, owned by the context): no slices, one pass.  196 B per signature (key and Jacobian record), the two
 * partial levels (196 B per partial: n / 16 and n / 256 partials, rounded up to runs of 32), 192 B per group and one word; for the
 * verifiers 34 B per signature, 291 B per message, three Fp12 records, the hash's workspace at m messages and the G2 MSM's at n terms;
 * for the aggregate form 98 B per committee and the workspace of zkp_g1_segment_sum_batch.
 *
 * Out of scope: sorting the signatures by message on the device (the caller sorts; the keys must arrive sorted), hashing to G1
 * (the 11-isogeny of RFC 9380), more than one GPU.  AggregateVerify with ragged numbers of messages per signature and G2 segment sums
 * went to zkp_bls_agg_g2.h.
 */
#ifndef ZKP_BLS_GROUPED_H
#define ZKP_BLS_GROUPED_H

#include "zkp_bls_agg.h"

#ifdef __cplusplus
extern "C" {
#endif

int zkp_g1_scaled_segment_sum_batch(zkp_ctx* ctx, const uint64_t* pts /* n x 12 */, const uint8_t* inf /* n or NULL */, const uint64_t* rand /* n x 2 */,
                                    size_t n, const uint64_t* seg_off /* n_seg + 1 */, size_t n_seg, uint64_t* out /* n_seg x 12 */,
                                    uint8_t* out_inf /* n_seg */, uint8_t* status /* n_seg */);
int zkp_g1_scaled_segment_sum_batch_dev(zkp_ctx* ctx, const void* d_pts, const void* d_inf, const void* d_rand, size_t n, const void* d_seg_off, size_t n_seg,
                                        void* d_out, void* d_out_inf, void* d_status, void* stream);
int zkp_bls_verify_grouped_batch(zkp_ctx* ctx, const uint64_t* pk /* n x 12 */, const uint8_t* inf_pk, const uint64_t* grp_off /* m + 1 */,
                                 const uint8_t* msgs, const uint64_t* offsets /* m + 1 */, size_t m, const uint8_t* dst, size_t dst_len,
                                 const uint64_t* sig /* n x 24 */, const uint8_t* inf_sig, size_t n, const uint64_t* rand /* n x 2 */, int flags, int* all_ok);
int zkp_bls_verify_grouped_batch_dev(zkp_ctx* ctx, const void* d_pk, const void* d_inf_pk, const void* d_grp_off, const void* d_msgs, const void* d_offsets,
                                     size_t m, const void* d_dst, size_t dst_len, const void* d_sig, const void* d_inf_sig, size_t n, const void* d_rand,
                                     int flags, void* d_all_ok, void* stream);
int zkp_bls_fast_aggregate_verify_grouped_batch(zkp_ctx* ctx, const uint64_t* table, size_t n_table, const uint32_t* idx, size_t n_idx,
                                                const uint64_t* seg_off /* n + 1 */, const uint64_t* grp_off /* m + 1 */, const uint8_t* msgs,
                                                const uint64_t* offsets /* m + 1 */, size_t m, const uint8_t* dst, size_t dst_len, const uint64_t* sig,
                                                const uint8_t* inf_sig, size_t n, const uint64_t* rand, int flags, int* all_ok);
int zkp_bls_fast_aggregate_verify_grouped_batch_dev(zkp_ctx* ctx, const void* d_table, size_t n_table, const void* d_idx, size_t n_idx, const void* d_seg_off,
                                                    const void* d_grp_off, const void* d_msgs, const void* d_offsets, size_t m, const void* d_dst,
                                                    size_t dst_len, const void* d_sig, const void* d_inf_sig, size_t n, const void* d_rand, int flags,
                                                    void* d_all_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif
