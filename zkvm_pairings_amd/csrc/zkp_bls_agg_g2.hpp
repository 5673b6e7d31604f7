// zkp_bls_agg_g2.hpp -- G2 segment sums, the min-sig FastAggregateVerify and AggregateVerify (zkp_bls_agg_g2.hip).  The functions take
// device pointers and arguments the C ABI has already checked, grow the context's aggregation workspace (ctxop::grow_agg) first and then
// only launch on `s`: asynchronous, nothing read back.
#pragma once
#include "zkp_rlc.hpp"

#include "zkp_bls_agg_g2_plan.hpp"

namespace zkp {

int agg2_segment_sum_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, void* out,
                         void* out_inf, void* status, hipStream_t s);
// flags: bit 0 = ZKP_BLS_POINTS_CHECKED
int agg2_minsig_verify_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* msgs,
                           const void* offsets, const void* dst, size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags,
                           int* all_ok, hipStream_t s);
int aggv_verify_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* msgs, const void* offsets, size_t n_msg, const void* seg_off, const void* dst,
                    size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s);

}  // namespace zkp
