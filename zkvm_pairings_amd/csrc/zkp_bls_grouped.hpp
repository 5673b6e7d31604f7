// zkp_bls_grouped.hpp -- scaled G1 segment sums and the BLS verifiers grouped by message (zkp_bls_grouped.hip).  Every function takes
// device pointers and arguments the C ABI has already checked, grows the context's workspaces first and then only launches on `s`:
// asynchronous, nothing read back.
#pragma once
#include "zkp_rlc.hpp"

#include "zkp_bls_grouped_plan.hpp"

namespace zkp {

namespace ctxop {
int grow_grp(zkp_ctx* c, size_t bytes, void** ws);     // the grow-only workspace of this file (zkp_bls_grouped_plan.hpp layout)
int grow_prod(zkp_ctx* c, size_t records);             // the Fp12 records of miller_product, grown before the first launch
}  // namespace ctxop

int grp_scaled_segment_sum_dev(zkp_ctx* c, const void* pts, const void* inf, const void* rand, size_t n, const void* seg_off, size_t n_seg, void* out,
                               void* out_inf, void* status, hipStream_t s);
// flags: bit 0 = ZKP_BLS_POINTS_CHECKED
int grp_verify_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* grp_off, const void* msgs, const void* offsets, size_t m, const void* dst,
                   size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s);
int grp_fast_aggregate_verify_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* grp_off,
                                  const void* msgs, const void* offsets, size_t m, const void* dst, size_t dst_len, const void* sig, const void* inf_sig,
                                  size_t n, const void* rand, int flags, int* all_ok, hipStream_t s);

}  // namespace zkp
