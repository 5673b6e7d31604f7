/*
 * include/zkp_bls_agg.h -- BLS committee aggregation of libzkp_pairings.so: sums of public keys gathered from a table by ragged index
 * lists, and FastAggregateVerify (one signature, one message, one committee per check) on top of them.  An eighth header of the SAME
 * library: include it beside zkp_bls.h, whose message layout (one byte buffer plus n + 1 offsets), DST argument, rand (2 u64 per
 * signature) and ZKP_BLS_POINTS_CHECKED it shares, and zkp_pairings.h (zkp_ctx, status codes, wire formats: G1 = 12 u64, G2 = 24 u64,
 * infinity bytes, the identity written as (0, 1), zkp_set_validate and the validation word).  Symbols added under ABI version 4
 * (zkp_abi_version() is still 4).
 *
 * Every entry point has a host-pointer flavour and a _dev flavour with a trailing stream.  The _dev flavour is asynchronous, reads nothing
 * back, and is capturable into a hipGraph once the context's workspaces have reached the call's size (run the call once before capturing
 * it) - the contract of zkp_bls_verify_batch_dev.
 *
 * Committees: a table of n_table FINITE affine G1 points in wire format (an identity is no public key: there is no table_inf), n_idx
 * entries idx[e] (u32: bits 0..30 the table row, bit 31 set: SUBTRACT the row), and n_seg + 1 offsets seg_off (u64): segment j is
 * idx[seg_off[j] .. seg_off[j + 1]).  The offsets are well formed when they are non-decreasing from seg_off[0] = 0 to
 * seg_off[n_seg] = n_idx.
 *
 * zkp_g1_segment_sum_batch               out[j] = sum over segment j of (+/-) table[row]: the affine wire point, canonical, so bit-exact
 *                                        whatever the order of addition; the identity is (0, 1) with out_inf = 1.  An empty segment is the
 *                                        identity with status 0; a row that occurs twice is doubled, not refused; +i and -i in one segment
 *                                        cancel.  The signed form is the sync-committee trick "the aggregate of all minus the absent": keep
 *                                        the total as one more table row.
 * zkp_bls_fast_aggregate_verify_batch    *all_ok = zkp_bls_verify_batch(apk, msgs, sig) with apk_j the segment sum of committee j, AND
 *                                        every status 0, AND no empty committee (FastAggregateVerify needs at least one key).  An
 *                                        aggregate that is the identity gives 0 (KeyValidate, the inf_pk of zkp_bls_verify_batch).  Unless
 *                                        flags has ZKP_BLS_POINTS_CHECKED, the AGGREGATES and the signatures go through is_valid; the table
 *                                        is the caller's, to be validated once with zkp_g1_is_valid_batch.  A non-zero status, an invalid
 *                                        point, a zero (a_i, b_i) give all_ok = 0, not an error.  n == 0 gives 1.
 *
 * Bad input, _dev flavour (the host sees nothing): a row at or above n_table is never used as an address; its segment comes out as the
 * identity with status = 1 and its neighbours are untouched.  Malformed offsets make the whole call malformed: every segment comes out as
 * the identity with status = 1 (the verifier: all_ok = 0), nothing outside idx[0 .. n_idx), seg_off[0 .. n_seg] and table[0 .. n_table)
 * is read, and in validation mode the validation word is ORed - the stance of zkp_hash_to_g2_batch_dev on its offsets.  The host
 * flavour, which sees both arrays, refuses both conditions with ZKP_ERR_ARG before a byte is copied.
 * ZKP_ERR_ARG in both flavours: null pointers with non-zero counts (seg_off counts n_seg + 1 values; the verifier's may be null when
 * n = 0 and n_idx = 0); n_table == 0 with n_idx > 0; n_table > 2^24; n_idx > 2^26 (every count of the accumulation stays in 32 bits:
 * there are no passes); n_seg > 2^24; for the verifier everything zkp_bls_verify_batch refuses.  Validation mode covers the table and
 * the signatures.
 *
 * How (zkvm_pairings_amd/csrc/zkp_bls_agg.hip, zkp_bls_agg_plan.hpp): the table goes to Montgomery records (k_msm_points); k_agg_zero
 * fills the call's word and the sums; k_agg_check tests the offsets and zeroes the statuses; k_agg_keys, a lane per entry, finds the
 * entry's segment by a bounded binary search (the sort key) and checks the row (the value); the bucket MSM's accumulation kernel
 * (k_msm_accum: 32 sorted entries per lane, mixed additions with every exceptional case of the group law, partial sums joined level by
 * level) sums them - the keys are sorted by construction, there is no sort -; k_agg_affine turns the Jacobian sums into affine points
 * with ONE inversion per wavefront of 64 sums (prefix and suffix products across the lanes through LDS).  The verifier then calls the
 * driver of zkp_bls_verify_batch on the sums and folds statuses and empty committees into all_ok (k_agg_fold): no second pairing path.
 * Cost: per entry one mixed addition (about 11 Fp products) and a 25-step search; per table row two conversions; per partial sum of a
 * level a full addition (16 products); per segment 18 products and 1/64 of an inversion of 461.  On one MI355X over a table of 2^20
 * keys: 1.7 ms for 2^14 committees of 64 keys, 1.8 ms for 2^11 of 512, 2.7 ms for one of 2^20.
 * Slices and workspace (grow-only, owned by the context): no slices, one pass.  128 B per table point, 8 B per entry, the two partial
 * levels (196 B per partial: n_idx / 16 and n_idx / 256 partials, rounded up to runs of 32), 192 B per segment and one word; for the
 * verifier 96 + 2 B per committee and the workspaces of zkp_bls_verify_batch.
 *
 * Out of scope: folding aggregates that sign the SAME message into one Miller pair (sum [r_i] apk_i by message before the pairing - the
 * follow-up, on this segment sum), aggregation bitfields expanded on the device, hashing to G1, more than one GPU.
 * G2 segment sums and AggregateVerify with ragged numbers of messages per signature went to zkp_bls_agg_g2.h.
 */
#ifndef ZKP_BLS_AGG_H
#define ZKP_BLS_AGG_H

#include "zkp_bls.h"

#ifdef __cplusplus
extern "C" {
#endif

int zkp_g1_segment_sum_batch(zkp_ctx* ctx, const uint64_t* table /* n_table x 12 */, size_t n_table, const uint32_t* idx /* n_idx */, size_t n_idx,
                             const uint64_t* seg_off /* n_seg + 1 */, size_t n_seg, uint64_t* out /* n_seg x 12 */, uint8_t* out_inf /* n_seg */,
                             uint8_t* status /* n_seg */);
int zkp_g1_segment_sum_batch_dev(zkp_ctx* ctx, const void* d_table, size_t n_table, const void* d_idx, size_t n_idx, const void* d_seg_off, size_t n_seg,
                                 void* d_out, void* d_out_inf, void* d_status, void* stream);
int zkp_bls_fast_aggregate_verify_batch(zkp_ctx* ctx, const uint64_t* table, size_t n_table, const uint32_t* idx, size_t n_idx, const uint64_t* seg_off,
                                        const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len, const uint64_t* sig /* n x 24 */,
                                        const uint8_t* inf_sig, size_t n, const uint64_t* rand /* n x 2 */, int flags, int* all_ok);
int zkp_bls_fast_aggregate_verify_batch_dev(zkp_ctx* ctx, const void* d_table, size_t n_table, const void* d_idx, size_t n_idx, const void* d_seg_off,
                                            const void* d_msgs, const void* d_offsets, const void* d_dst, size_t dst_len, const void* d_sig,
                                            const void* d_inf_sig, size_t n, const void* d_rand, int flags, void* d_all_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif
