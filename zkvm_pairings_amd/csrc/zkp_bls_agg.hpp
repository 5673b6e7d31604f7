// zkp_bls_agg.hpp -- G1 segment sums and FastAggregateVerify (zkp_bls_agg.hip).  Both functions take device pointers and arguments the C
// ABI has already checked, grow the context's workspace first and then only launch on `s`: asynchronous, nothing read back.
#pragma once
#include "zkp_rlc.hpp"

#include "zkp_bls_agg_plan.hpp"

namespace zkp {

namespace ctxop {
int grow_agg(zkp_ctx* c, size_t bytes, void** ws);     // the grow-only workspace of this file (zkp_bls_agg_plan.hpp layout)
}  // namespace ctxop

int agg_segment_sum_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, void* out, void* out_inf,
                        void* status, hipStream_t s);
// flags: bit 0 = ZKP_BLS_POINTS_CHECKED
int agg_verify_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* msgs, const void* offsets,
                   const void* dst, size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s);

}  // namespace zkp
