// zkp_cells.hpp -- the KZG cell proofs (zkp_cells.hip): FK20 multi-proofs on cosets.  They borrow the context's fk20 workspace and its
// domain and split tables through zkp_fk20.hpp's ctxop, and the transforms' launch descriptors from zkp_fk20.hip.
#pragma once
#include "zkp_fk20.hpp"

#include "zkp_cells_plan.hpp"

namespace zkp {

// the calls on device pointers, asynchronous on s, arguments already checked: they grow the context's workspaces first, then only launch
int cells_setup_dev(zkp_ctx* c, const uint64_t* monomial, unsigned log2_n, unsigned log2_l, uint64_t* out, uint8_t* out_inf, hipStream_t s);
int cells_dev(zkp_ctx* c, const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* coeffs, size_t n, unsigned log2_n, unsigned log2_l, unsigned log2_ext,
              int flags, uint64_t* out_proof, uint8_t* out_inf, hipStream_t s);

// the verifier on device pointers: *all_ok (device int32), asynchronous on s
struct CellBatch {
    const uint64_t *monomial, *g2, *tau_l_g2, *c, *values, *proof, *rand;
    const uint8_t *inf_c, *inf_proof;
    const uint32_t* index;
    size_t n;
    unsigned log2_d, log2_l;
};
int cell_check_dev(zkp_ctx* c, const CellBatch& b, int flags, int* all_ok, hipStream_t s);

}  // namespace zkp
