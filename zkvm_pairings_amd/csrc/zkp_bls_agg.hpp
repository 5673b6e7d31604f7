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

// the launches of this unit's fill and index kernels, for zkp_bls_agg_g2.hip: k_agg_zero over `bytes` (a multiple of 16) from p; k_agg_check
// (word zeroed before; zeroes status[0 .. n_seg)); k_agg_keys (no launch when n_idx = 0); k_agg_fold
namespace aggk {
int zero(zkp_ctx* c, void* p, size_t bytes, hipStream_t s);
int check(zkp_ctx* c, const void* seg_off, size_t n_seg, size_t n_idx, uint8_t* status, int* word, hipStream_t s);
int keys(zkp_ctx* c, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, size_t n_table, const int* word, uint32_t* keys, uint32_t* vals,
         uint8_t* status, hipStream_t s);
int fold(zkp_ctx* c, const uint8_t* status, const void* seg_off, size_t n, const int* word, int* all_ok, hipStream_t s);
}  // namespace aggk

}  // namespace zkp
