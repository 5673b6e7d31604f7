// zkp_recover.hpp -- the cell recovery (zkp_recover.hip): erased blobs back from half their cells.  It borrows the context's kzg
// workspace, its domain table and its coset tables through zkp_poly.hpp's ctxop, and the Fr transform and inversion launchers.
#pragma once
#include "zkp_poly.hpp"

#include "zkp_recover_plan.hpp"

namespace zkp {

// ORs 1 into *bad when a value of a PRESENT cell is >= r (rows = n M cells of 2^log2_l values); the bytes of a missing cell are not read
hipError_t rec_check_present(const uint64_t* values, const uint8_t* present, size_t rows, unsigned log2_l, int* bad, hipStream_t s);
// the call on device pointers, asynchronous on s, arguments already checked: it grows the context's workspace first, then only launches
int recover_dev(zkp_ctx* c, const uint64_t* values, const uint8_t* present, size_t n, unsigned log2_n, unsigned log2_l, int flags, uint64_t* out_coeffs,
                int32_t* out_ok, hipStream_t s);

}  // namespace zkp
