// zkp_bls.hpp -- hash-to-G2 and the BLS batch verifier (zkp_bls.hip).  Every function takes device pointers and arguments the C ABI has
// already checked, grows the context's workspace first and then only launches on `s`: asynchronous, nothing read back.
#pragma once
#include "zkp_rlc.hpp"

#include "zkp_bls_plan.hpp"

namespace zkp {

namespace ctxop {
int grow_bls(zkp_ctx* c, size_t bytes, void** ws);     // the grow-only workspace of this file (zkp_bls_plan.hpp layout)
int* bls_bad_word(zkp_ctx* c);                         // the sticky validation word in validation mode, null otherwise
}  // namespace ctxop

int h2c_wide_dev(zkp_ctx* c, const void* bytes, size_t n, void* out, hipStream_t s);
int h2c_field_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out_u, hipStream_t s);
int h2c_map_dev(zkp_ctx* c, const void* u, size_t n, void* out, void* out_inf, hipStream_t s);
int h2c_clear_dev(zkp_ctx* c, const void* pts, const void* inf, size_t n, void* out, void* out_inf, hipStream_t s);
int h2c_hash_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out, void* out_inf, hipStream_t s);
// flags: bit 0 = ZKP_BLS_POINTS_CHECKED
int bls_verify_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig,
                   const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s);

}  // namespace zkp
