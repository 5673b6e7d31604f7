// zkp_rlc.hpp -- the random-linear-combination batch check (zkp_rlc.hip) and what it borrows from the context (zkp_pairings.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/zkp_pairings.h"

namespace zkp {

// the context's pieces the driver composes, each launch-only on `s` (zkp_pairings.hip)
namespace ctxop {
int fail(zkp_ctx* c, const char* what, hipError_t e);                         // ZKP_OK, or the error noted in the context
int grow_rlc(zkp_ctx* c, size_t bytes, void** ws);                            // the grow-only RLC workspace
int grow_msm(zkp_ctx* c, size_t bytes);                                       // the grow-only MSM workspace
int msm(zkp_ctx* c, int which, const void* pts, const void* inf, const void* sc, size_t m, size_t n_msm, void* out, void* out_inf, hipStream_t s);
int valid(zkp_ctx* c, int which, const void* pts, const void* inf, size_t n, void* status, hipStream_t s);
int miller_product(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n, uint64_t* out, hipStream_t s);
// *is_one = (final_exponentiation(f_0 ... f_{n-1}) == 1); f is destroyed, gt receives the Gt value
int gt_is_one(zkp_ctx* c, uint64_t* f, size_t n, uint64_t* gt, int* is_one, hipStream_t s);
}  // namespace ctxop

// the batch check on device pointers (arguments already checked): *all_ok (device int32) = AND of every check, asynchronous on s
int rlc_check_dev(zkp_ctx* c, const zkp_rlc_batch* b, const uint64_t* rand, int flags, int* all_ok, hipStream_t s);

}  // namespace zkp
