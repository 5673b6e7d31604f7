/*
 * include/zkp_bls_agg_g2.h -- G2 aggregation of libzkp_pairings.so: sums of G2 points gathered from a table by ragged index lists -
 * signature aggregation in the min-pk layout, key aggregation in the min-sig layout -, FastAggregateVerify for committees of G2 keys, and
 * AggregateVerify (one signature over several (key, message) pairs), the third verifier of the BLS draft.  An eleventh header of the SAME
 * library: include it beside zkp_bls_agg.h and zkp_bls_minsig.h, whose conventions it shares to the letter: entries idx[e] (u32: bits
 * 0..30 the table row, bit 31 set: SUBTRACT the row), n_seg + 1 offsets seg_off (u64), well formed when non-decreasing from seg_off[0] = 0
 * to the entry count; the message layout (one byte buffer plus offsets), DST, rand (2 u64 per check), ZKP_BLS_POINTS_CHECKED and the
 * validation word of zkp_bls.h; the wire formats of zkp_pairings.h (G1 = 12 u64, G2 = 24 u64, infinity bytes, the identity written as
 * (0, 1)).  Symbols added under ABI version 4 (zkp_abi_version() is still 4).  This is where the G2 segment sums and the AggregateVerify
 * that zkp_bls_agg.h, zkp_bls_grouped.h and zkp_bls_minsig.h name as out of scope went.
 *
 * Every entry point has a host-pointer flavour and a _dev flavour with a trailing stream.  The _dev flavour is asynchronous, reads nothing
 * back, and is capturable into a hipGraph once the context's workspaces have reached the call's size (run the call once before capturing
 * it) - the contract of zkp_bls_verify_batch_dev.
 *
 * zkp_g2_segment_sum_batch                     out[j] = sum over segment j of (+/-) table[row]: the affine wire point, canonical, so
 *                                              bit-exact whatever the order of addition; the identity is (0, 1) with out_inf = 1.  The
 *                                              rules of zkp_g1_segment_sum_batch: an empty segment is the identity with status 0; a row
 *                                              that occurs twice is doubled; +i and -i cancel.  The table holds n_table FINITE points (there
 *                                              is no table_inf), any canonical points of the twist y^2 = x^3 + 4 (1 + u): rows outside G2
 *                                              are summed by the curve's law, validating the table is the caller's job
 *                                              (zkp_g2_is_valid_batch).
 * zkp_bls_minsig_fast_aggregate_verify_batch   the arguments of zkp_bls_fast_aggregate_verify_batch with the table n_table x 24 and sig
 *                                              n x 12.  *all_ok = the min-sig batch verifier's answer (zkp_bls_minsig.h) on (apk,
 *                                              msgs, sig) with apk_j the G2 segment sum of committee j, AND every status 0, AND no empty committee.  An aggregate that is the
 *                                              identity gives 0.  Unless flags has ZKP_BLS_POINTS_CHECKED, the AGGREGATES and the
 *                                              signatures go through is_valid.  n == 0 gives 1.
 * zkp_bls_aggregate_verify_batch               min-pk AggregateVerify, batched: signature j (G2) covers the pairs (pk_i, m_i) for i in
 *                                              [seg_off[j], seg_off[j + 1]); pk, inf_pk, msgs and offsets hold n_msg rows, sig, inf_sig and
 *                                              rand hold n.  *all_ok = zkp_bls_verify_batch(pk, msgs, sig', inf_sig', rand') where for
 *                                              message i of segment j rand'_i = rand_j and sig'_i = sig_j if i == seg_off[j], the flagged
 *                                              identity otherwise; AND the offsets are well formed; AND no segment is empty (the draft
 *                                              requires at least one pair).  By bilinearity that is prod_j [prod_i e([r_j] pk_i, H(m_i))]
 *                                              e(-g1, [r_j] sig_j) == 1: one hash and one Miller pair per message, one G2 MSM over the
 *                                              signatures, one final exponentiation.  Messages within a segment are NOT tested for
 *                                              distinctness: this is the AggregateVerify of the proof-of-possession scheme; the basic
 *                                              scheme's rule that the messages of one signature differ stays with the caller.  An identity
 *                                              among the keys, an invalid point, a zero rand row give 0, not an error.  n == 0 with
 *                                              n_msg == 0 gives 1; n == 0 with n_msg > 0 is malformed.
 *
 * Bad input, _dev flavour (the host sees nothing): a row at or above n_table is never used as an address; its segment comes out as the
 * identity with status = 1 and its neighbours are untouched.  Malformed offsets make the whole call malformed: every segment comes out as
 * the identity with status = 1 (the verifiers: all_ok = 0), nothing outside the arrays is read, and in validation mode the validation
 * word is ORed.  The host flavour, which sees the arrays, refuses both conditions with ZKP_ERR_ARG before a byte is copied.
 * ZKP_ERR_ARG in both flavours: null pointers with non-zero counts (seg_off counts n_seg + 1 values; the verifiers' may be null when every
 * count is 0; inf_pk and inf_sig may be null: no infinities); n_table == 0 with n_idx > 0; n_table > 2^24 (4 GB of Montgomery records);
 * n_idx > 2^26; n_seg > 2^24; for the committee verifier everything the min-sig batch verifier refuses; for AggregateVerify everything
 * zkp_bls_verify_batch refuses on n_msg, and n > 2^24.  Validation mode covers the table, the keys and the signatures.
 *
 * How (zkvm_pairings_amd/csrc/zkp_bls_agg_g2.hip, zkp_bls_agg_g2_plan.hpp): the table goes to Montgomery records (k_msm_points on
 * 4 n_table field elements); the fill, the check of the offsets and the keys are the kernels of zkp_bls_agg.h (k_agg_zero, k_agg_check,
 * k_agg_keys); the bucket MSM's accumulation kernel on G2 (k_msm_accum<2>, two lanes per point) sums the entries level by level;
 * k_agg2_affine, a lane per sum, turns the Jacobian sums into affine points with ONE Fp inversion per wavefront of 64 sums: the chain of
 * prefix and suffix products runs over the norms z0^2 + z1^2, then 1 / Z = conj(Z) / N.  The committee verifier calls the driver of
 * the min-sig batch verifier on the sums and folds statuses and empty committees into all_ok (k_agg_fold).  AggregateVerify expands
 * signatures and rand rows per message into workspace rows (k_aggv_expand, a lane per message with the bounded search of k_agg_keys),
 * calls the driver of zkp_bls_verify_batch unchanged and folds empty segments: no second pairing path.
 * Cost: per entry one mixed G2 addition and a 25-step search; per table row four conversions; per partial sum a full addition; per segment
 * about 34 Fp products and 1/64 of an inversion of 461; AggregateVerify: what zkp_bls_verify_batch costs on n_msg messages plus 209 B
 * written per message.  On one MI355X over a table of 2^20 points (tools/time_agg_g2.py, medians of 3): the sum takes 2.46 ms for
 * 2^14 segments of 64, 2.66 ms for 2^11 of 512, 3.77 ms for one of 2^20, against 3.67 / 4.08 / 4.94 ms of a gather and a zkp_g2_add_batch_dev
 * tree; the committee verifier 23.8 and 23.2 ms at the first two shapes, 21.3 and 20.5 ms of which are the min-sig verifier on precomputed
 * aggregates; AggregateVerify 295.0 / 295.8 / 275.3 ms at 2^14 x 64, 2^11 x 512 and 1 x 2^20 pairs, against 295.3 / 295.7 / 274.0 ms of
 * zkp_bls_verify_batch_dev on arrays expanded outside the timing: the expansion costs 0.5 % at the most.
 * Slices and workspace (grow-only, owned by the context, the aggregation workspace of zkp_bls_agg.h): no slices, one pass.  256 B per
 * table point, 8 B per entry, the two partial levels (388 B per partial: n_idx / 16 and n_idx / 256 partials, rounded up to runs of 32),
 * 384 B per segment and one word; for the committee verifier 192 + 2 B per committee and the workspaces of the min-sig batch verifier;
 * for AggregateVerify 209 B per message, 1 B per signature and the workspaces of zkp_bls_verify_batch.
 *
 * Out of scope: grouping by message for the min-sig layout, sorting or deduplicating messages on the device, aggregation bitfields
 * expanded on the device, a table_inf, more than one GPU.
 */
#ifndef ZKP_BLS_AGG_G2_H
#define ZKP_BLS_AGG_G2_H

#include "zkp_bls.h"

#ifdef __cplusplus
extern "C" {
#endif

int zkp_g2_segment_sum_batch(zkp_ctx* ctx, const uint64_t* table /* n_table x 24 */, size_t n_table, const uint32_t* idx /* n_idx */, size_t n_idx,
                             const uint64_t* seg_off /* n_seg + 1 */, size_t n_seg, uint64_t* out /* n_seg x 24 */, uint8_t* out_inf /* n_seg */,
                             uint8_t* status /* n_seg */);
int zkp_g2_segment_sum_batch_dev(zkp_ctx* ctx, const void* d_table, size_t n_table, const void* d_idx, size_t n_idx, const void* d_seg_off, size_t n_seg,
                                 void* d_out, void* d_out_inf, void* d_status, void* stream);
int zkp_bls_minsig_fast_aggregate_verify_batch(zkp_ctx* ctx, const uint64_t* table /* n_table x 24 */, size_t n_table, const uint32_t* idx, size_t n_idx,
                                               const uint64_t* seg_off, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                                               const uint64_t* sig /* n x 12 */, const uint8_t* inf_sig, size_t n, const uint64_t* rand /* n x 2 */,
                                               int flags, int* all_ok);
int zkp_bls_minsig_fast_aggregate_verify_batch_dev(zkp_ctx* ctx, const void* d_table, size_t n_table, const void* d_idx, size_t n_idx, const void* d_seg_off,
                                                   const void* d_msgs, const void* d_offsets, const void* d_dst, size_t dst_len, const void* d_sig,
                                                   const void* d_inf_sig, size_t n, const void* d_rand, int flags, void* d_all_ok, void* stream);
int zkp_bls_aggregate_verify_batch(zkp_ctx* ctx, const uint64_t* pk /* n_msg x 12 */, const uint8_t* inf_pk, const uint8_t* msgs,
                                   const uint64_t* offsets /* n_msg + 1 */, size_t n_msg, const uint64_t* seg_off /* n + 1 */, const uint8_t* dst,
                                   size_t dst_len, const uint64_t* sig /* n x 24 */, const uint8_t* inf_sig, size_t n, const uint64_t* rand /* n x 2 */,
                                   int flags, int* all_ok);
int zkp_bls_aggregate_verify_batch_dev(zkp_ctx* ctx, const void* d_pk, const void* d_inf_pk, const void* d_msgs, const void* d_offsets, size_t n_msg,
                                       const void* d_seg_off, const void* d_dst, size_t dst_len, const void* d_sig, const void* d_inf_sig, size_t n,
                                       const void* d_rand, int flags, void* d_all_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif
