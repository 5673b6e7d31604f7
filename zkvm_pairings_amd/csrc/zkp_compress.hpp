// zkp_compress.hpp -- host-side launchers of zkp_compress.hip (compressed point codec and the square-root hooks), called by the
// C ABI in zkp_pairings.hip.  Every launcher enqueues its kernel on `s` and returns the launch status; n <= 2^31 - 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace zkp_cmp {

// which = 1 (G1: 48 B in, 12 u64 out) or 2 (G2: 96 B in, 24 u64 out); status: zkp_point_status 0..3
hipError_t decompress(int which, const void* bytes, size_t n, void* out, void* out_inf, void* status, hipStream_t s);
// inf may be NULL (no infinities)
hipError_t compress(int which, const void* pts, const void* inf, size_t n, void* out_bytes, hipStream_t s);
// which = 1: Fp::sqrt (6 u64 per element); which = 2: Fp2::sqrt (12 u64).  out = the reference's root or zero, is_square 0 / 1
hipError_t sqrt_ref(int which, const uint64_t* a, size_t n, uint64_t* out, uint8_t* is_square, hipStream_t s);

}  // namespace zkp_cmp
