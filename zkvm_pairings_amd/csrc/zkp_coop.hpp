// zkp_coop.hpp -- interface between the C-ABI dispatcher (zkp_pairings.hip) and the
// lane-cooperative kernel family (zkp_coop.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "zkp_cells_plan.hpp"
#include "zkp_fk20_plan.hpp"

namespace zkp {

struct CoopState {
    bool available = false;
    int cus = 0;
    void* d_prog = nullptr;   // microcode tables resident in HBM
    void* d_ws = nullptr;     // per-launch workspace (Miller outputs between the two phases)
    size_t ws_bytes = 0;
};

hipError_t coop_init(CoopState* st, const hipDeviceProp_t& prop);
void coop_free(CoopState* st);
// true when `kind` (zkp_kernel_kind) routes the pairing path through the cooperative kernels
bool coop_selected(const CoopState* st, int kind);
// pairs per check the cooperative path takes (checks with more than eight pairs run in groups of eight)
bool coop_supports_k(size_t k);
// batched Fp operation on wire operands through the 28-bit core: op 0 mul, 1 add, 2 sub, 3 neg, 4 square, 5 invert
hipError_t coop_fp28_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, hipStream_t s);
// G1/G2 is_valid on the 28-bit core (status 0 / 1 / 2)
hipError_t coop_g1_valid(const uint64_t* g1, const uint8_t* inf, size_t n, uint8_t* status, hipStream_t s);
// st: the context's cooperative state (the three-wave G2 kernel keeps the affine points' limbs in a scratch buffer of its own)
hipError_t coop_g2_valid(CoopState* st, const uint64_t* g2, const uint8_t* inf, size_t n, uint8_t* status, hipStream_t s);
hipError_t coop_g1_mul(const uint64_t* base, size_t stride, const uint64_t* sc, size_t n, uint64_t* out, uint8_t* out_inf, hipStream_t s);
hipError_t coop_g2_mul(const uint64_t* base, size_t stride, const uint64_t* sc, size_t n, uint64_t* out, uint8_t* out_inf, hipStream_t s);
// out[i] = a[i] + b[i] on the 28-bit core, which = 1 (G1) or 2 (G2); ia / ib / out_inf may be null
hipError_t coop_add(int which, const uint64_t* a, const uint8_t* ia, const uint64_t* b, const uint8_t* ib, size_t n, uint64_t* out, uint8_t* out_inf,
                    hipStream_t s);
// hash-to-G2: out[i] = [h_eff] P_i with P_i the wire point i (pts non-null; inf may be null) or the sum of the homogeneous projective points in
// slots 2 i and 2 i + 1 of ws (pts null; layout at k_h2c_clear, zkp_bls_clear.hip)
hipError_t coop_h2c_clear(const uint64_t* pts, const uint8_t* inf, const int32_t* ws, size_t stride, size_t n, uint64_t* out, uint8_t* out_inf, hipStream_t s);
// out[i] = [a] P_i + [b] (beta x_i, -y_i) with (a, b) = ab[2 (i / per)], ab[2 (i / per) + 1] (= [a + b z^2] P_i in G1); inf / out_inf may be null
hipError_t coop_g1_mul_endo(const uint64_t* base, const uint8_t* inf, const uint64_t* ab, size_t n, uint32_t per, uint64_t* out, uint8_t* out_inf,
                            hipStream_t s);
// rec[i] = [a_i + b_i z^2] P_i as Jacobian records (192 B each) with (a_i, b_i) = ab[2 i], ab[2 i + 1]: the input of msm_accum(1, false, ...);
// inf may be null (zkp_bls_grouped.hip)
hipError_t grp_scale(const uint64_t* base, const uint8_t* inf, const uint64_t* ab, uint32_t n, void* rec, hipStream_t s);
// the bucket MSM's launches (zkp_coop.hip, "group addition and bucket MSM"; driven by zkp_msm.hip, sized by zkp_msm_plan.hpp)
hipError_t msm_points(const uint64_t* w, uint32_t n_fp, void* rec, hipStream_t s);
hipError_t msm_digits(const uint64_t* sc, const uint8_t* inf, uint32_t terms, uint32_t m, int shared, uint32_t c, uint32_t windows, uint32_t* keys,
                      uint32_t* vals, hipStream_t s);
hipError_t msm_accum(int which, bool level0, const uint32_t* keys, const uint32_t* vals, const void* src, uint32_t n, uint32_t n_sums, void* sums,
                     uint32_t* okeys, void* oj, hipStream_t s);
hipError_t msm_reduce(int which, const void* buckets, uint32_t n_sums, uint32_t split, uint32_t chunk, uint32_t* okeys, void* oj, hipStream_t s);
hipError_t msm_final(int which, const void* wsums, uint32_t segs, uint32_t windows, uint32_t c, uint64_t* out, uint8_t* out_inf, hipStream_t s);
// the G1 NTT's and FK20's group launches (zkp_coop.hip, "the G1 NTT"; driven by zkp_fk20.hip, every index from zkp_fk20_plan.hpp).  rec: the
// Jacobian records; split: the context's split twiddles (a_lo, a_hi, b_lo, b_hi per entry); ab: the four words of the scaling's split (a.scale: one more launch)
hipError_t g1ntt_first(const uint64_t* in, const uint8_t* inf, void* rec, const fk20::First& a, hipStream_t s);
hipError_t g1ntt_stage(void* rec, const uint64_t* split, const fk20::Stage& a, hipStream_t s);
hipError_t g1ntt_out(void* rec, uint64_t* out, uint8_t* out_inf, const fk20::Out& a, const uint64_t* ab, hipStream_t s);
hipError_t fk20_mul(const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* sc, uint32_t n_pt, uint32_t k1, void* rec, hipStream_t s);
// the cell proofs' multiply-accumulate and the sum of its partials (zkp_coop.hip, "the KZG cell proofs"; driven by zkp_cells.hip, every index from
// zkp_cells_plan.hpp).  part: the Jacobian partials (unused when g = l), rec: the blocks of records
hipError_t cell_mac(const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* sc, void* part, void* rec, const cells::Mac& a, hipStream_t s);
hipError_t cell_sum(const void* part, void* rec, const cells::Sum& a, hipStream_t s);
// one tower operation per record (zkp_tower_op_batch); ab = n a-records followed by n b-records
hipError_t coop_tower_op(CoopState* st, int op, const uint64_t* ab, size_t n, uint32_t repeat, uint64_t* out, hipStream_t s);
hipError_t coop_time_prog(CoopState* st, int which, size_t n, hipStream_t s, hipEvent_t e0, hipEvent_t e1, float* ms);
hipError_t coop_miller(CoopState* st, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n_checks,
                       size_t k, uint64_t* out, hipStream_t s);
// out (wire Gt), ok (per element Gt == identity) and all_ok (AND-ed into *all_ok) are each optional
hipError_t coop_final_exp(CoopState* st, const uint64_t* f, size_t n, uint64_t* out, uint8_t* ok, int* all_ok, hipStream_t s);
// one level of the Fp12 product tree, in place on wire records: buf[c] <- buf[c] * buf[c + h] for c < m
hipError_t coop_fp12_mul_pairs(CoopState* st, uint64_t* buf, size_t m, size_t h, hipStream_t s);
// n_dev (device pointer, may be null): the number of checks that exist, <= n_checks, read by the kernels themselves (never by the host)
hipError_t coop_pairing(CoopState* st, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n_checks,
                        size_t k, uint64_t* out_gt, uint8_t* ok, int* all_ok, hipStream_t s, const uint32_t* n_dev = nullptr);

// measurement: one pass of the fused pairing, ms / launches per kernel class (ZKP_PROFILE_CLASSES of them, include/zkp_pairings.h)
hipError_t coop_profile_pairing(CoopState* st, const uint64_t* g1, const uint64_t* g2, size_t n, uint64_t* out_gt, float* ms, int* launches, hipStream_t s);

}  // namespace zkp

// debugging aid: ZKP_DEBUG_ALLOC=<file> appends one line per device / pinned allocation and release (address, bytes, what for), so
// that the address of a GPU memory fault can be matched to a buffer
#include <cstdio>
#include <cstdlib>
#include <string>
static inline void zkp_dbg_alloc(const char* what, const void* p, size_t bytes) {
    static const std::string path = getenv("ZKP_DEBUG_ALLOC") ? getenv("ZKP_DEBUG_ALLOC") : "";   // a copy: setenv may move the environment
    if (path.empty()) return;
    if (FILE* f = fopen(path.c_str(), "a")) {
        fprintf(f, "%s %p %zu\n", what, p, bytes);
        fclose(f);
    }
}
