// zkp_bls_agg.hip -- BLS committee aggregation on the GPU (gfx950): sums of gathered, signed G1 table rows per segment of a ragged list
// (zkp_g1_segment_sum_batch) and FastAggregateVerify on top of them (zkp_bls_fast_aggregate_verify_batch).
//
//   k_agg_zero    the fill of the call's word and of the Jacobian sums (a kernel, not a memset node: DESIGN 3.2)
//   k_agg_check   one lane per offset pair: seg_off[0] = 0, non-decreasing, seg_off[n_seg] = n_idx, or the call's word is set; the
//                 statuses are zeroed
//   k_agg_keys    one lane per entry: key = the entry's segment by a bounded search in seg_off, value = row | sign; a row at or above
//                 n_table marks its segment and becomes row 0; a malformed call gives every entry msm::KEY_NONE
//   k_agg_affine  the Jacobian sums to affine wire points, ONE inversion per wavefront (Montgomery's trick across the 64 lanes)
//   k_agg_fold    the verifier's: a set status, an empty committee or a malformed call stores 0 to all_ok
// Between k_agg_keys and k_agg_affine the sums are the bucket MSM's: msm_points converts the table, msm_accum (k_msm_accum, zkp_coop.hip)
// runs the levels of the run-wise segmented sum exactly as msm_run drives them.  The keys are sorted by construction: there is no sort.
//
// tests/agg_kernel_host.cpp compiles the index kernels (k_agg_check, k_agg_keys) for the host (ZKP_AGG_KERNELS_ONLY) under sanitizers and
// runs them as written on exactly allocated buffers.
#ifndef ZKP_AGG_KERNELS_ONLY
#include "zkp_bls_agg.hpp"

#include "zkp_bls.hpp"
#include "zkp_coop.hpp"
#include "zkp_fp28_ext.hpp"
#else
#include "zkp_bls_agg_plan.hpp"
#endif

namespace zkp {
namespace {

constexpr int TPB_I = 256;   // the index kernels
constexpr int TPB_A = 64;    // k_agg_affine: a wavefront per workgroup, the wavefront is the unit of the shared inversion

// ------------------------------------------------------------------------------------------- the index kernels
// lane j <= n_seg: the pair (seg_off[j], seg_off[j + 1]), lane n_seg the two ends.  word: the call's "malformed" word (zeroed by k_agg_zero
// before); bad: the validation word, null outside validation mode.  Reads seg_off[0 .. n_seg] only.
__global__ void __launch_bounds__(TPB_I) k_agg_check(const uint64_t* seg_off, uint32_t n_seg, uint64_t n_idx, uint8_t* status, int* word, int* bad) {
    const uint32_t j = blockIdx.x * TPB_I + threadIdx.x;
    if (j > n_seg) return;
    bool wrong;
    if (j < n_seg) {
        status[j] = 0;
        wrong = seg_off[j + 1] < seg_off[j];
    } else {
        wrong = seg_off[0] != 0 || seg_off[n_seg] != n_idx;
    }
    if (wrong) {
        atomicOr(word, 1);
        if (bad) atomicOr(bad, 1);
    }
}

// lane e < n_idx.  Sound offsets put e in exactly one segment j with seg_off[j] <= e < seg_off[j + 1]; the search keeps
// seg_off[lo] <= e < seg_off[hi] with 0 <= lo < hi <= n_seg, so it reads seg_off[1 .. n_seg - 1] only and ends within SEARCH_STEPS.
__global__ void __launch_bounds__(TPB_I) k_agg_keys(const uint32_t* idx, uint32_t n_idx, const uint64_t* seg_off, uint32_t n_seg, uint32_t n_table,
                                                    const int* word, uint32_t* keys, uint32_t* vals, uint8_t* status) {
    const uint32_t e = blockIdx.x * TPB_I + threadIdx.x;
    if (e >= n_idx) return;
    if (*word) {
        keys[e] = msm::KEY_NONE;
        vals[e] = 0;
        return;
    }
    uint32_t lo = 0, hi = n_seg;
    for (int step = 0; step < agg::SEARCH_STEPS && hi - lo > 1; step++) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (seg_off[mid] <= e) lo = mid; else hi = mid;
    }
    const uint32_t v = idx[e];
    uint32_t row = v & agg::ROW_MASK;
    if (row >= n_table) {
        status[lo] = 1;                  // every writer stores the same 1
        row = 0;                         // a row that exists (n_table > 0 whenever there is an entry)
    }
    keys[e] = lo;
    vals[e] = row | (v & agg::SIGN);
}

#ifndef ZKP_AGG_KERNELS_ONLY
using zkp28::Fp28;
using zkp28::NL;
using namespace zkp_f28;

__global__ void k_agg_zero(uint4* p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = make_uint4(0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------- Jacobian sums -> affine wire points
// a Montgomery record of 64 bytes (rec_store of zkp_coop.hip): 14 limbs in four int4
__device__ __forceinline__ void rec_ld(Fp28& x, const int4* src) {
    const int4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
    x.l[0] = v0.x; x.l[1] = v0.y; x.l[2] = v0.z; x.l[3] = v0.w; x.l[4] = v1.x; x.l[5] = v1.y; x.l[6] = v1.z; x.l[7] = v1.w;
    x.l[8] = v2.x; x.l[9] = v2.y; x.l[10] = v2.z; x.l[11] = v2.w; x.l[12] = v3.x; x.l[13] = v3.y;
}
// a value per lane in LDS, plane pl (limb quad q of lane l at [(pl * 4 + q) * 64 + l]: a lane's four stores and loads are conflict-free)
__device__ __forceinline__ void sh_st(int4* sh, int pl, int lane, const Fp28& x) {
    sh[(pl * 4 + 0) * 64 + lane] = make_int4(x.l[0], x.l[1], x.l[2], x.l[3]);
    sh[(pl * 4 + 1) * 64 + lane] = make_int4(x.l[4], x.l[5], x.l[6], x.l[7]);
    sh[(pl * 4 + 2) * 64 + lane] = make_int4(x.l[8], x.l[9], x.l[10], x.l[11]);
    sh[(pl * 4 + 3) * 64 + lane] = make_int4(x.l[12], x.l[13], 0, 0);
}
__device__ __forceinline__ void sh_ld(Fp28& x, const int4* sh, int pl, int lane) {
    const int4 v0 = sh[(pl * 4 + 0) * 64 + lane], v1 = sh[(pl * 4 + 1) * 64 + lane], v2 = sh[(pl * 4 + 2) * 64 + lane], v3 = sh[(pl * 4 + 3) * 64 + lane];
    x.l[0] = v0.x; x.l[1] = v0.y; x.l[2] = v0.z; x.l[3] = v0.w; x.l[4] = v1.x; x.l[5] = v1.y; x.l[6] = v1.z; x.l[7] = v1.w;
    x.l[8] = v2.x; x.l[9] = v2.y; x.l[10] = v2.z; x.l[11] = v2.w; x.l[12] = v3.x; x.l[13] = v3.y;
}
__device__ __forceinline__ void f_pick(Fp28& r, const Fp28& a, bool take) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = take ? a.l[i] : r.l[i];
}

// One lane per sum, a wavefront per workgroup.  1 / Z_l for the 64 sums of a wavefront from ONE inversion: inclusive prefix products
// P_l = z_0 .. z_l and suffix products S_l = z_l .. z_63 by six doubling steps each through LDS (two independent products per step), then
// 1 / z_l = P_(l-1) S_(l+1) / P_63.  A sum at infinity (Z = 0 by the predicate of zkp_coop.hip: the stored limbs are not canonical, the
// test canonicalises), a sum whose status is set and every sum of a malformed call enter the chain as 1 and come out as the identity
// (0, 1) with out_inf = 1, so the shared product is never zero.  Per lane 12 + 2 products of the chain and 4 of the affine point beside
// the wavefront's 461; the wire words are the canonical values of X / Z^2 and Y / Z^3, the ones jac_affine gives.
// The final status is written here: status | word.
__global__ void __launch_bounds__(TPB_A) k_agg_affine(const int4* sums, uint32_t n_seg, const int* word, uint8_t* status, uint64_t* out, uint8_t* out_inf) {
    __shared__ int4 sh[2 * 4 * 64];
    const int lane = threadIdx.x;
    const uint32_t j = blockIdx.x * TPB_A + lane;
    const bool live = j < n_seg;
    const uint32_t jj = live ? j : n_seg - 1;
    const int4* rec = sums + (size_t)jj * 12;
    const bool refused = *word || (live && status[j]);
    Fp28 one, z;
    f_const(one, zkp28::K28_ONE);
    rec_ld(z, rec + 8);
    const bool dead = !live || refused || f_is_zero(z);
    f_pick(z, one, dead);
    Fp28 pre = z, suf = z;
#pragma unroll 1
    for (int d = 1; d < 64; d *= 2) {
        sh_st(sh, 0, lane, pre);
        sh_st(sh, 1, lane, suf);
        __syncthreads();
        const bool dn = lane >= d, up = lane + d < 64;
        Fp28 a, b;
        sh_ld(a, sh, 0, dn ? lane - d : lane);
        sh_ld(b, sh, 1, up ? lane + d : lane);
        __syncthreads();
        f_mul(a, pre, a);
        f_mul(b, suf, b);
        f_pick(pre, a, dn);
        f_pick(suf, b, up);
    }
    sh_st(sh, 0, lane, pre);
    sh_st(sh, 1, lane, suf);
    __syncthreads();
    Fp28 total, before = one, after = one, zi, zi2, t, ax, ay;
    sh_ld(total, sh, 0, 63);
    sh_ld(t, sh, 0, lane ? lane - 1 : 0);
    f_pick(before, t, lane > 0);
    sh_ld(t, sh, 1, lane < 63 ? lane + 1 : 63);
    f_pick(after, t, lane < 63);
    f_mul(before, before, after);
    {   // 1 / total = (total^((p-3)/4))^4 total
        Fp28 e;
        f_pow_exp(e, total);
        f_sqr(e, e);
        f_sqr(e, e);
        f_mul(t, e, total);
    }
    f_mul(zi, before, t);
    f_sqr(zi2, zi);
    rec_ld(t, rec);
    f_mul(ax, t, zi2);
    f_mul(zi2, zi2, zi);
    rec_ld(t, rec + 4);
    f_mul(ay, t, zi2);
    if (!live) return;
    uint64_t wx[6], wy[6];
    zkp28::fp28_to_wire(wx, ax);
    zkp28::fp28_to_wire(wy, ay);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        out[12 * (size_t)j + k] = dead ? 0 : wx[k];
        out[12 * (size_t)j + 6 + k] = dead ? (k == 0 ? 1 : 0) : wy[k];
    }
    out_inf[j] = dead ? 1 : 0;
    status[j] = refused ? 1 : 0;
}

// committee i refuses the batch when its status is set or it is empty; lane 0 also when the call is malformed (which sets every status,
// but a call of no committee has none).  Every writer stores the same 0: a plain store, as k_bls_fold's.
__global__ void __launch_bounds__(TPB_I) k_agg_fold(const uint8_t* status, const uint64_t* seg_off, uint32_t n, const int* word, int* all_ok) {
    const uint32_t i = blockIdx.x * TPB_I + threadIdx.x;
    if (i == 0 && *word) *all_ok = 0;
    if (i < n && (status[i] || seg_off[i + 1] == seg_off[i])) *all_ok = 0;
}

inline unsigned blocks_of(size_t n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

#define AGG_CHK(c, what, call)                                        \
    do {                                                              \
        if (int rc__ = ctxop::fail((c), (what), (call))) return rc__; \
    } while (0)

// the six steps on a workspace of layout L; out / out_inf / status: device, n_seg rows
int sums_into(zkp_ctx* c, const agg::Layout& L, char* w, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg,
              uint64_t* out, uint8_t* out_inf, uint8_t* status, hipStream_t s) {
    int* word = (int*)(w + L.word);
    uint32_t *keys = (uint32_t*)(w + L.keys), *vals = (uint32_t*)(w + L.vals);
    uint32_t* part_k[2] = {(uint32_t*)(w + L.part_k[0]), (uint32_t*)(w + L.part_k[1])};
    void* part_j[2] = {w + L.part_j[0], w + L.part_j[1]};
    AGG_CHK(c, "k_msm_points", msm_points((const uint64_t*)table, (uint32_t)(2 * n_table), w + L.pts, s));
    {   // the word and the sums in one fill, before the check that may set the word
        const size_t n16 = L.fill / 16, want = (n16 + 255) / 256;
        hipLaunchKernelGGL(k_agg_zero, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, s, (uint4*)word, n16);
        AGG_CHK(c, "k_agg_zero", hipGetLastError());
    }
    hipLaunchKernelGGL(k_agg_check, dim3(blocks_of(n_seg + 1, TPB_I)), dim3(TPB_I), 0, s, (const uint64_t*)seg_off, (uint32_t)n_seg, (uint64_t)n_idx, status, word,
                       ctxop::bls_bad_word(c));
    AGG_CHK(c, "k_agg_check", hipGetLastError());
    if (n_idx) {
        hipLaunchKernelGGL(k_agg_keys, dim3(blocks_of(n_idx, TPB_I)), dim3(TPB_I), 0, s, (const uint32_t*)idx, (uint32_t)n_idx, (const uint64_t*)seg_off,
                           (uint32_t)n_seg, (uint32_t)n_table, (const int*)word, keys, vals, status);
        AGG_CHK(c, "k_agg_keys", hipGetLastError());
    }
    // level 0 from the entries, then the partial sums ping-pong until one run is left (msm_run's loop)
    uint32_t n = (uint32_t)n_idx;
    const uint32_t* kin = keys;
    const void* jin = w + L.pts;
    for (int lv = 0; n; lv++) {
        AGG_CHK(c, "k_msm_accum", msm_accum(1, lv == 0, kin, vals, jin, n, (uint32_t)n_seg, w + L.sums, part_k[lv & 1], part_j[lv & 1], s));
        if (n <= msm::RUN) break;
        n = 2 * msm::runs_of(n);
        kin = part_k[lv & 1];
        jin = part_j[lv & 1];
    }
    if (n_seg) {
        hipLaunchKernelGGL(k_agg_affine, dim3(blocks_of(n_seg, TPB_A)), dim3(TPB_A), 0, s, (const int4*)(w + L.sums), (uint32_t)n_seg, (const int*)word, status, out,
                           out_inf);
        AGG_CHK(c, "k_agg_affine", hipGetLastError());
    }
    return 0;
}

}  // namespace

int agg_segment_sum_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, void* out, void* out_inf,
                        void* status, hipStream_t s) {
    if (!n_seg && !n_idx) return 0;
    const agg::Layout L = agg::layout(n_table, n_idx, n_seg, false);
    void* ws = nullptr;
    if (int rc = ctxop::grow_agg(c, L.total, &ws)) return rc;
    return sums_into(c, L, (char*)ws, table, n_table, idx, n_idx, seg_off, n_seg, (uint64_t*)out, (uint8_t*)out_inf, (uint8_t*)status, s);
}

int agg_verify_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* msgs, const void* offsets,
                   const void* dst, size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s) {
    if (!n && !n_idx) return bls_verify_dev(c, nullptr, nullptr, msgs, offsets, dst, dst_len, sig, inf_sig, 0, rand, flags, all_ok, s);   // the empty batch holds
    const agg::Layout L = agg::layout(n_table, n_idx, n, true);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_agg(c, L.total, &ws))) return rc;
    char* w = (char*)ws;
    uint64_t* apk = (uint64_t*)(w + L.apk);
    uint8_t *apk_inf = (uint8_t*)(w + L.apk_inf), *st = (uint8_t*)(w + L.st);
    // the sums (with n = 0 still the check of the offsets: a call of no committee and some entries is malformed)
    if ((rc = sums_into(c, L, w, table, n_table, idx, n_idx, seg_off, n, apk, apk_inf, st, s))) return rc;
    if ((rc = bls_verify_dev(c, apk, apk_inf, msgs, offsets, dst, dst_len, sig, inf_sig, n, rand, flags, all_ok, s))) return rc;
    hipLaunchKernelGGL(k_agg_fold, dim3(blocks_of(n ? n : 1, TPB_I)), dim3(TPB_I), 0, s, (const uint8_t*)st, (const uint64_t*)seg_off, (uint32_t)n,
                       (const int*)(w + L.word), all_ok);
    return ctxop::fail(c, "k_agg_fold", hipGetLastError());
}

// the fill and the index kernels for zkp_bls_agg_g2.hip, which indexes G2 tables and message lists by the same rules
namespace aggk {
int zero(zkp_ctx* c, void* p, size_t bytes, hipStream_t s) {
    const size_t n16 = bytes / 16, want = (n16 + 255) / 256;
    hipLaunchKernelGGL(k_agg_zero, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, s, (uint4*)p, n16);
    return ctxop::fail(c, "k_agg_zero", hipGetLastError());
}
int check(zkp_ctx* c, const void* seg_off, size_t n_seg, size_t n_idx, uint8_t* status, int* word, hipStream_t s) {
    hipLaunchKernelGGL(k_agg_check, dim3(blocks_of(n_seg + 1, TPB_I)), dim3(TPB_I), 0, s, (const uint64_t*)seg_off, (uint32_t)n_seg, (uint64_t)n_idx, status, word,
                       ctxop::bls_bad_word(c));
    return ctxop::fail(c, "k_agg_check", hipGetLastError());
}
int keys(zkp_ctx* c, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, size_t n_table, const int* word, uint32_t* keys, uint32_t* vals,
         uint8_t* status, hipStream_t s) {
    if (!n_idx) return 0;
    hipLaunchKernelGGL(k_agg_keys, dim3(blocks_of(n_idx, TPB_I)), dim3(TPB_I), 0, s, (const uint32_t*)idx, (uint32_t)n_idx, (const uint64_t*)seg_off,
                       (uint32_t)n_seg, (uint32_t)n_table, word, keys, vals, status);
    return ctxop::fail(c, "k_agg_keys", hipGetLastError());
}
int fold(zkp_ctx* c, const uint8_t* status, const void* seg_off, size_t n, const int* word, int* all_ok, hipStream_t s) {
    hipLaunchKernelGGL(k_agg_fold, dim3(blocks_of(n ? n : 1, TPB_I)), dim3(TPB_I), 0, s, status, (const uint64_t*)seg_off, (uint32_t)n, word, all_ok);
    return ctxop::fail(c, "k_agg_fold", hipGetLastError());
}
}  // namespace aggk

#else
}  // namespace
#endif

}  // namespace zkp
