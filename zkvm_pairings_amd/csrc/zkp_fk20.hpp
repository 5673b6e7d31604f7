// zkp_fk20.hpp -- the G1 NTT and the FK20 proofs (zkp_fk20.hip), and what they borrow from the context (zkp_pairings.hip) beside
// zkp_poly.hpp's ctxop.
#pragma once
#include "zkp_poly.hpp"

#include "zkp_fk20_plan.hpp"

namespace zkp {

namespace ctxop {
int grow_fk20(zkp_ctx* c, size_t bytes, void** ws);
// the split twiddles of the domain of at least 2^log2_n points (a, b of 128 bits with w^t = a + b z^2 mod r), kept by the context, grow-only,
// built on `s` from the domain table whenever that table grows.  Also hands out the domain table itself.
int g1ntt_tables(zkp_ctx* c, unsigned log2_n, const uint32_t** domain, const uint64_t** split, unsigned* table_log2, hipStream_t s);
}  // namespace ctxop

// split[i] <- the split of domain[i], i < 2^log2_n
hipError_t g1ntt_split_build(const uint32_t* domain, unsigned log2_n, uint64_t* split, hipStream_t s);
// the launch descriptors of a transform and its twiddled stages 1 .. k - 1, shared with the cell proofs (zkp_cells.hip)
int run_stages(zkp_ctx* c, void* rec, const uint64_t* split, unsigned table_log2, const fk20::Span& at, bool inverse, hipStream_t s);
fk20::First first_of(const fk20::Span& at, uint32_t mode, bool perm, uint32_t src_off);
fk20::Out out_of(const fk20::Span& at, bool perm, bool scale);
// the three calls on device pointers, asynchronous on s, arguments already checked: they grow the context's workspaces first, then only launch
int g1_ntt_dev(zkp_ctx* c, const uint64_t* points, const uint8_t* inf, size_t n_vec, unsigned log2_n, int flags, uint64_t* out, uint8_t* out_inf, hipStream_t s);
int fk20_setup_dev(zkp_ctx* c, const uint64_t* monomial, unsigned log2_n, uint64_t* out, uint8_t* out_inf, hipStream_t s);
int fk20_dev(zkp_ctx* c, const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* coeffs, size_t n, unsigned log2_n, int flags, uint64_t* out_proof,
             uint8_t* out_inf, hipStream_t s);

}  // namespace zkp
