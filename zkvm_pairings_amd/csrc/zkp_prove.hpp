// zkp_prove.hpp -- the Fr sparse matrix-vector product, the QAP quotient and the batched Groth16 prover (zkp_prove.hip), and what they
// borrow from the context (zkp_pairings.hip) beside zkp_poly.hpp's ctxop.
#pragma once
#include "../../include/zkp_prove.h"
#include "zkp_poly.hpp"

namespace zkp {

namespace ctxop {
int grow_prove(zkp_ctx* c, size_t bytes, void** ws);   // the grow-only workspace of the quotient and the prover (zkp_prove_plan.hpp layout)
int* validation_word(zkp_ctx* c);                       // the sticky word of the _dev calls (device int32)
// [sc_i] base_i (stride 0: one base) and a_i + b_i of n G1 (which = 1) or G2 (which = 2) points: the launch code of zkp_g*_mul_batch /
// zkp_g*_add_batch
int mul(zkp_ctx* c, int which, const void* base, size_t stride, const void* sc, size_t n, void* out, void* out_inf, hipStream_t s);
int add(zkp_ctx* c, int which, const void* a, const void* inf_a, const void* b, const void* inf_b, size_t n, void* out, void* out_inf, hipStream_t s);
}  // namespace ctxop

// launch-only on device pointers, arguments already checked (n >= 1, out_stride >= 1); brv_log2 != 0 stores row k at slot
// bitrev(k, brv_log2) (out_stride = 2^brv_log2 then); bad: ORed with 1 when the matrix points outside its arrays
hipError_t fr_spmv(const zkp_fr_csr* mat, const uint64_t* x, size_t n, size_t out_stride, unsigned brv_log2, uint64_t* out, int* bad, hipStream_t s);
// the two calls on device pointers, asynchronous on s: they grow the context's workspaces first, then only launch
int groth16_quotient_dev(zkp_ctx* c, const zkp_r1cs* r, const uint64_t* witness, size_t n, uint64_t* out_h, uint8_t* out_sat, hipStream_t s);
int groth16_prove_dev(zkp_ctx* c, const zkp_r1cs* r, const zkp_groth16_pk* pk, const uint64_t* witness, const uint64_t* rs, size_t n, uint64_t* out_a,
                      uint8_t* out_inf_a, uint64_t* out_b, uint8_t* out_inf_b, uint64_t* out_c, uint8_t* out_inf_c, uint8_t* out_sat, hipStream_t s);

}  // namespace zkp
