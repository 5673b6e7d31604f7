// zkp_poly.hpp -- the batched Fr NTT and the KZG opening (zkp_poly.hip), and what they borrow from the context (zkp_pairings.hip)
// beside zkp_kzg.hpp's ctxop.
#pragma once
#include "zkp_kzg.hpp"

namespace zkp {

namespace ctxop {
// the coset tables 7^j, 7^(2^10 j), 7^-j, 7^-(2^10 j) (j < 2^10, Montgomery form), kept by the context and built on `s` at the first use
int poly_coset(zkp_ctx* c, const uint32_t** coset, hipStream_t s);
}  // namespace ctxop

// launch-only pieces on device pointers, arguments already checked
hipError_t poly_coset_build(uint32_t* coset, hipStream_t s);   // poly::COSET_BYTES
// ws: poly::ntt_workspace_bytes(n_poly, log2_n, flags) bytes (may be null when that is 0); coset may be null without ZKP_NTT_COSET;
// out == in is allowed; n_poly >= 1
hipError_t fr_ntt(void* ws, const uint32_t* table, unsigned table_log2, const uint32_t* coset, const uint64_t* in, size_t n_poly, unsigned log2_n, int flags,
                  uint64_t* out, hipStream_t s);
// the opening on device pointers, asynchronous on s: grows the context's workspaces first, then only launches
int kzg_open_dev(zkp_ctx* c, const void* lagrange, const uint64_t* evals, const uint64_t* z, size_t n, unsigned log2_n, int flags, uint64_t* out_y,
                 uint64_t* out_proof, uint8_t* out_inf, hipStream_t s);

}  // namespace zkp
