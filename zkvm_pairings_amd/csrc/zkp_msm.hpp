// zkp_msm.hpp -- host driver of the bucket multi-scalar multiplication (zkp_msm.hip), called by the C ABI in zkp_pairings.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace zkp {

constexpr int MSM_PHASES = 6;   // points, digits, sort, accumulate, reduce (+ fix-up), final

// device workspace one call of msm_run needs (which = 1: G1, 2: G2); 0 when the sizes are outside the ABI
size_t msm_workspace_bytes(int which, size_t m, size_t n_msm, int shared);
// n_msm sums of m terms, enqueued on s: no host synchronisation, no allocation.  ws: msm_workspace_bytes of device memory.
// phase_ms (measurement only, may be null): the call synchronises and adds each phase's milliseconds, summed over the passes.
hipError_t msm_run(int which, void* ws, const uint64_t* points, const uint8_t* inf, const uint64_t* scalars, size_t m, size_t n_msm, int shared,
                   uint64_t* out, uint8_t* out_inf, hipStream_t s, float* phase_ms = nullptr);

}  // namespace zkp
