// zkp_groth16.hpp -- Fr arithmetic, the Fr fold and the batched Groth16 verifier (zkp_groth16.hip), and the one more thing they borrow
// from the context (zkp_pairings.hip) beside zkp_rlc.hpp's ctxop.
#pragma once
#include "zkp_rlc.hpp"

namespace zkp {

namespace ctxop {
int grow_g16(zkp_ctx* c, size_t bytes, void** ws);                            // the grow-only workspace of the fold and the verifier
}  // namespace ctxop

// launch-only pieces on device pointers, arguments already checked (n >= 1)
hipError_t fr_check_canonical(const uint64_t* a, size_t n, int* bad, hipStream_t s);   // ORs 1 into *bad when an element is >= r
hipError_t fr_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, hipStream_t s);
hipError_t fr_from_wide(const uint8_t* bytes, size_t n, uint64_t* out, hipStream_t s);
// out[i] = sum_c w_c x_{c,i} mod r (l of them), *sum_w = sum_c w_c mod r (may be null); part / sum_part: the partial accumulators of
// g16::fold_plan(n, l); ok (may be null): ok[0] is cleared when an x is >= r
hipError_t fr_fold(void* part, void* sum_part, const uint64_t* w, const uint64_t* x, size_t n, size_t l, uint64_t* out, uint64_t* sum_w, int* ok,
                   hipStream_t s);
// the verifier on device pointers: *all_ok (device int32), asynchronous on s
int groth16_check_dev(zkp_ctx* c, const zkp_groth16_vk* vk, const zkp_groth16_batch* b, const uint64_t* rand, int flags, int* all_ok, hipStream_t s);

}  // namespace zkp
