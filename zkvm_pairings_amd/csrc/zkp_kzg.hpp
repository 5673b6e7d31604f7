// zkp_kzg.hpp -- the batched Fr inversion, the barycentric evaluation and the batch KZG opening verifier (zkp_kzg.hip), and what they
// borrow from the context (zkp_pairings.hip) beside zkp_rlc.hpp's and zkp_groth16.hpp's ctxop.
#pragma once
#include "zkp_groth16.hpp"

namespace zkp {

namespace ctxop {
// n_msm sums over the SAME m points: scalars row by row (zkp_g1_msm_batch's shared_bases)
int msm_shared(zkp_ctx* c, int which, const void* pts, const void* inf, const void* sc, size_t m, size_t n_msm, void* out, void* out_inf, hipStream_t s);
int grow_kzg(zkp_ctx* c, size_t bytes, void** ws);   // the grow-only workspace of the three calls (zkp_kzg_plan.hpp layouts)
// the domain table omega_K^i (i < 2^K, Montgomery form) for some K >= log2_n, kept by the context and rebuilt on `s` only when
// log2_n exceeds what it holds: omega_k^i is entry i << (*table_log2 - log2_n)
int kzg_domain(zkp_ctx* c, unsigned log2_n, const uint32_t** table, unsigned* table_log2, hipStream_t s);
}  // namespace ctxop

// launch-only pieces on device pointers, arguments already checked
hipError_t fr_domain_build(uint32_t* table, unsigned log2_n, hipStream_t s);
// out[i] = a[i]^-1, 0 for 0; out == a is allowed; ws: kzg::inv_plan(n).total bytes; n >= 1
hipError_t fr_invert(void* ws, const uint64_t* a, size_t n, uint64_t* out, hipStream_t s);
// ws: kzg::eval_layout(n_poly, log2_n).total bytes; n_poly >= 1
hipError_t fr_eval(void* ws, const uint32_t* table, unsigned table_log2, const uint64_t* evals, const uint64_t* z, size_t n_poly, unsigned log2_n, int flags,
                   uint64_t* out, hipStream_t s);
// the verifier's small launches, shared with the cell verifier (zkp_cells.hip): flag[0] = 1, flag[1] = 0 (n_zero: *all_ok = 1 instead);
// any non-zero status byte clears flag[0]; out = -g2 | tau_g2, the G2 side of the two pairs; *all_ok = flag[0] && flag[1]
hipError_t kzg_flag_init(int* flag, int* all_ok, int n_zero, hipStream_t s);
hipError_t kzg_flag_status(const uint8_t* st, size_t n, int* flag, hipStream_t s);
hipError_t kzg_g2_side(const uint64_t* g2, const uint64_t* tau_g2, uint64_t* out, hipStream_t s);
hipError_t kzg_flag_finish(const int* flag, int* all_ok, hipStream_t s);
// the verifier on device pointers: *all_ok (device int32), asynchronous on s
int kzg_check_dev(zkp_ctx* c, const zkp_kzg_vk* vk, const zkp_kzg_batch* b, const uint64_t* rand, int flags, int* all_ok, hipStream_t s);

}  // namespace zkp
