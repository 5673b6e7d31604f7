// zkp_bls_minsig.hpp -- hash-to-G1 and the minimal-signature-size BLS batch verifiers (zkp_bls_minsig.hip).  Every function takes device
// pointers and arguments the C ABI has already checked, grows the context's workspace first and then only launches on `s`:
// asynchronous, nothing read back.
#pragma once
#include "zkp_bls.hpp"

#include "zkp_bls_minsig_plan.hpp"

namespace zkp {

namespace ctxop {
int grow_minsig(zkp_ctx* c, size_t bytes, void** ws);  // the grow-only workspace of this file (zkp_bls_minsig_plan.hpp layout)
}  // namespace ctxop

int g1h_field_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out_u, hipStream_t s);
int g1h_map_dev(zkp_ctx* c, const void* u, size_t n, void* out, void* out_inf, hipStream_t s);
int g1h_clear_dev(zkp_ctx* c, const void* pts, const void* inf, size_t n, void* out, void* out_inf, hipStream_t s);
int g1h_hash_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out, void* out_inf, hipStream_t s);
// flags: bit 0 = ZKP_BLS_POINTS_CHECKED
int minsig_verify_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig,
                      const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s);
int minsig_verify_samekey_dev(zkp_ctx* c, const void* pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig,
                              const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s);

}  // namespace zkp
