// zkp_bls_grouped.hip -- BLS verification grouped by message on the GPU (gfx950): sums of SCALED G1 points per segment of an ordered list
// (zkp_g1_scaled_segment_sum_batch), the batch verifier that folds the signatures of one message into one Miller pair
// (zkp_bls_verify_grouped_batch) and its FastAggregateVerify form (zkp_bls_fast_aggregate_verify_grouped_batch).
//
//     prod_i e([r_i] pk_i, H(m_g(i)))  =  prod_g e(A_g, H(m_g)),   A_g = sum_{i in group g} [r_i] pk_i,   r_i = a_i + b_i z^2
//
//   k_grp_zero     the fill of the call's word and of the Jacobian sums (a kernel, not a memset node: DESIGN 3.2)
//   k_grp_check    one lane per offset pair: seg_off[0] = 0, non-decreasing, seg_off[n_seg] = n, or the call's word is set; the statuses
//                  are zeroed
//   k_grp_keys     one lane per point: key = the point's segment by a bounded search in seg_off, with msm::KEY_FLAG (a scaled key is a
//                  partial sum that "holds a real contribution"); a malformed call gives every point msm::KEY_NONE
//   k_grp_scale    (zkp_coop.hip, beside k_g1_mul_endo28) [a_i + b_i z^2] P_i as a Jacobian record at the point's own index
//   k_grp_affine   the Jacobian sums to affine wire points, ONE inversion per wavefront (the scheme of k_agg_affine)
//   k_grp_init, k_grp_scalars, k_grp_fold, k_grp_committees, k_grp_finish, k_grp_set    the verifier's flags
// Between k_grp_scale and k_grp_affine the sums are the bucket MSM's: msm_accum(1, false, ...) (k_msm_accum, zkp_coop.hip) runs the levels
// of the run-wise segmented sum on Jacobian records exactly as msm_run and zkp_bls_agg.hip drive them (msm::level_chain).  The keys are
// sorted by construction: there is no sort.
//
// tests/grp_kernel_host.cpp compiles the index kernels (k_grp_check, k_grp_keys) for the host (ZKP_GRP_KERNELS_ONLY) under sanitizers and
// runs them as written on exactly allocated buffers.
#ifndef ZKP_GRP_KERNELS_ONLY
#include "zkp_bls_grouped.hpp"

#include "zkp_bls.hpp"
#include "zkp_bls_agg.hpp"
#include "zkp_coop.hpp"
#include "zkp_fp28_ext.hpp"
#include "zkp_msm.hpp"
#include "zkp_rlc_plan.hpp"
#else
#include "zkp_bls_grouped_plan.hpp"
#endif

namespace zkp {
namespace {

constexpr int TPB_I = 256;   // the index and flag kernels
constexpr int TPB_A = 64;    // k_grp_affine: a wavefront per workgroup, the wavefront is the unit of the shared inversion

// ------------------------------------------------------------------------------------------- the index kernels
// lane j <= n_seg: the pair (seg_off[j], seg_off[j + 1]), lane n_seg the two ends.  word: the call's "malformed" word (zeroed by k_grp_zero
// before); bad: the validation word, null outside validation mode.  Reads seg_off[0 .. n_seg] only.
__global__ void __launch_bounds__(TPB_I) k_grp_check(const uint64_t* seg_off, uint32_t n_seg, uint64_t n, uint8_t* status, int* word, int* bad) {
    const uint32_t j = blockIdx.x * TPB_I + threadIdx.x;
    if (j > n_seg) return;
    bool wrong;
    if (j < n_seg) {
        status[j] = 0;
        wrong = seg_off[j + 1] < seg_off[j];
    } else {
        wrong = seg_off[0] != 0 || seg_off[n_seg] != n;
    }
    if (wrong) {
        atomicOr(word, 1);
        if (bad) atomicOr(bad, 1);
    }
}

// lane i < n.  Sound offsets put i in exactly one segment j with seg_off[j] <= i < seg_off[j + 1]; the search keeps
// seg_off[lo] <= i < seg_off[hi] with 0 <= lo < hi <= n_seg, so it reads seg_off[1 .. n_seg - 1] only and ends within SEARCH_STEPS.
__global__ void __launch_bounds__(TPB_I) k_grp_keys(uint32_t n, const uint64_t* seg_off, uint32_t n_seg, const int* word, uint32_t* keys) {
    const uint32_t i = blockIdx.x * TPB_I + threadIdx.x;
    if (i >= n) return;
    if (*word) {
        keys[i] = msm::KEY_NONE;
        return;
    }
    uint32_t lo = 0, hi = n_seg;
    for (int step = 0; step < grp::SEARCH_STEPS && hi - lo > 1; step++) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (seg_off[mid] <= i) lo = mid; else hi = mid;
    }
    keys[i] = lo | msm::KEY_FLAG;
}

#ifndef ZKP_GRP_KERNELS_ONLY
using zkp28::Fp28;
using zkp28::NL;
using namespace zkp_f28;

__global__ void k_grp_zero(uint4* p, size_t n16) {
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

// One lane per sum, a wavefront per workgroup: k_agg_affine's scheme (that kernel sits in the unnamed namespace of zkp_bls_agg.hip, whose
// text a CPU gate pins).  1 / Z_l for the 64 sums of a wavefront from ONE inversion: inclusive prefix products P_l = z_0 .. z_l and suffix
// products S_l = z_l .. z_63 by six doubling steps each through LDS, then 1 / z_l = P_(l-1) S_(l+1) / P_63.  A sum at infinity (Z = 0: a
// segment nothing was added to keeps the fill's zeros, a sum that cancelled holds a zero Z of k_msm_accum) and every sum of a malformed call
// enter the chain as 1 and come out as the identity (0, 1) with out_inf = 1, so the shared product is never zero.  The wire words are the
// canonical values of X / Z^2 and Y / Z^3, the ones jac_affine gives.  The final status is written here: the call's word.
__global__ void __launch_bounds__(TPB_A) k_grp_affine(const int4* sums, uint32_t n_seg, const int* word, uint8_t* status, uint64_t* out, uint8_t* out_inf) {
    __shared__ int4 sh[2 * 4 * 64];
    const int lane = threadIdx.x;
    const uint32_t j = blockIdx.x * TPB_A + lane;
    const bool live = j < n_seg;
    const uint32_t jj = live ? j : n_seg - 1;
    const int4* rec = sums + (size_t)jj * 12;
    const bool refused = *word != 0;
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

// ------------------------------------------------------------------------------------------- the verifier's small kernels
// flag[0] = 0 (nothing refuses the batch yet), flag[1] = 0 (the product is not known to be one); -g1 as a wire point
__global__ void k_grp_init(int* flag, uint64_t* neg_g1, uint8_t* neg_g1_inf) {
    if (blockIdx.x || threadIdx.x) return;
    flag[0] = 0;
    flag[1] = 0;
    Fp28 x, y;
    f_const(x, zkp28::K28_G1_X);
    f_const(y, zkp28::K28_G1_Y);
    f_neg(y, y);
    zkp28::fp28_to_wire(neg_g1, x);
    zkp28::fp28_to_wire(neg_g1 + 6, y);
    *neg_g1_inf = 0;
}
// any non-zero byte (a status of the points check, an identity among the public keys) refuses the batch (every writer stores the same 1)
__global__ void __launch_bounds__(TPB_I) k_grp_fold(const uint8_t* st, size_t n, int* flag) {
    const size_t i = (size_t)blockIdx.x * TPB_I + threadIdx.x;
    if (i < n && st[i]) flag[0] = 1;
}
// sc[4 i ..] = a_i + b_i z^2 as the MSM's 4-word integer; a zero (a, b) would drop its signature: it refuses the batch
__global__ void __launch_bounds__(TPB_I) k_grp_scalars(const uint64_t* rand, size_t n, uint64_t* sc, int* flag) {
    const size_t i = (size_t)blockIdx.x * TPB_I + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = rand[2 * i], b = rand[2 * i + 1];
    if (!a && !b) flag[0] = 1;
    uint64_t r[rlc::SCALAR_U64];
    rlc::scalar(a, b, r);
    for (size_t w = 0; w < rlc::SCALAR_U64; w++) sc[i * rlc::SCALAR_U64 + w] = r[w];
}
// FastAggregateVerify: committee i refuses the batch when its status is set or it is empty (k_agg_fold's rule)
__global__ void __launch_bounds__(TPB_I) k_grp_committees(const uint8_t* status, const uint64_t* seg_off, uint32_t n, int* flag) {
    const uint32_t i = blockIdx.x * TPB_I + threadIdx.x;
    if (i < n && (status[i] || seg_off[i + 1] == seg_off[i])) flag[0] = 1;
}
__global__ void k_grp_finish(const int* flag, const int* word, int* all_ok) { *all_ok = (!flag[0] && !*word && flag[1]) ? 1 : 0; }
__global__ void k_grp_set(int* all_ok, int v) { *all_ok = v; }

inline unsigned blocks_of(size_t n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

#define GRP_CHK(c, what, call)                                        \
    do {                                                              \
        if (int rc__ = ctxop::fail((c), (what), (call))) return rc__; \
    } while (0)

// the sums on a workspace of layout L; out / out_inf / status: device, n_seg rows
int sums_into(zkp_ctx* c, const grp::Layout& L, char* w, const void* pts, const void* inf, const void* rand, size_t n, const void* seg_off, size_t n_seg,
              uint64_t* out, uint8_t* out_inf, uint8_t* status, hipStream_t s) {
    int* word = (int*)(w + L.word);
    uint32_t* keys = (uint32_t*)(w + L.keys);
    uint32_t* part_k[2] = {(uint32_t*)(w + L.part_k[0]), (uint32_t*)(w + L.part_k[1])};
    void* part_j[2] = {w + L.part_j[0], w + L.part_j[1]};
    {   // the word and the sums in one fill, before the check that may set the word
        const size_t n16 = L.fill / 16, want = (n16 + 255) / 256;
        hipLaunchKernelGGL(k_grp_zero, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, s, (uint4*)word, n16);
        GRP_CHK(c, "k_grp_zero", hipGetLastError());
    }
    hipLaunchKernelGGL(k_grp_check, dim3(blocks_of(n_seg + 1, TPB_I)), dim3(TPB_I), 0, s, (const uint64_t*)seg_off, (uint32_t)n_seg, (uint64_t)n, status, word,
                       ctxop::bls_bad_word(c));
    GRP_CHK(c, "k_grp_check", hipGetLastError());
    if (n) {
        hipLaunchKernelGGL(k_grp_keys, dim3(blocks_of(n, TPB_I)), dim3(TPB_I), 0, s, (uint32_t)n, (const uint64_t*)seg_off, (uint32_t)n_seg, (const int*)word, keys);
        GRP_CHK(c, "k_grp_keys", hipGetLastError());
        GRP_CHK(c, "k_grp_scale", grp_scale((const uint64_t*)pts, (const uint8_t*)inf, (const uint64_t*)rand, (uint32_t)n, w + L.jrec, s));
    }
    // every level reads Jacobian records: the scaled keys, then the partial sums ping-pong until one run is left (msm_run's loop)
    uint32_t cnt = (uint32_t)n;
    const uint32_t* kin = keys;
    const void* jin = w + L.jrec;
    for (int lv = 0; cnt; lv++) {
        GRP_CHK(c, "k_msm_accum", msm_accum(1, /*level0=*/false, kin, nullptr, jin, cnt, (uint32_t)n_seg, w + L.sums, part_k[lv & 1], part_j[lv & 1], s));
        if (cnt <= msm::RUN) break;
        cnt = 2 * msm::runs_of(cnt);
        kin = part_k[lv & 1];
        jin = part_j[lv & 1];
    }
    if (n_seg) {
        hipLaunchKernelGGL(k_grp_affine, dim3(blocks_of(n_seg, TPB_A)), dim3(TPB_A), 0, s, (const int4*)(w + L.sums), (uint32_t)n_seg, (const int*)word, status, out,
                           out_inf);
        GRP_CHK(c, "k_grp_affine", hipGetLastError());
    }
    return 0;
}

// every workspace the verifier touches, before its first launch (an allocation synchronises the device)
int grow_all(zkp_ctx* c, size_t n, size_t m, size_t extra, void** ws) {
    int rc;
    void* bls_ws = nullptr;
    if ((rc = ctxop::grow_grp(c, grp::layout(n, m, true).total + extra, ws)) || (rc = ctxop::grow_bls(c, bls::layout(m, false).total, &bls_ws)) ||
        (rc = ctxop::grow_msm(c, msm_workspace_bytes(2, n, 1, 0))) || (rc = ctxop::grow_prod(c, m / 8 + 1)))
        return rc;
    return 0;
}

// the nine steps on a workspace of layout L.  com_st / com_off: FastAggregateVerify's statuses and committee offsets (n of them), or null
int verify_into(zkp_ctx* c, const grp::Layout& L, char* w, const void* pk, const void* inf_pk, const void* grp_off, const void* msgs, const void* offsets,
                size_t m, const void* dst, size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, const uint8_t* com_st,
                const void* com_off, int* all_ok, hipStream_t s) {
    int rc;
    int* flag = (int*)(w + L.flag);
    uint8_t* st = (uint8_t*)(w + L.st);
    uint64_t *sc = (uint64_t*)(w + L.sc), *apk = (uint64_t*)(w + L.apk), *hq = (uint64_t*)(w + L.hq), *ml = (uint64_t*)(w + L.ml);
    uint64_t *neg_g1 = (uint64_t*)(w + L.neg_g1), *ssum = (uint64_t*)(w + L.s);
    uint8_t *apk_inf = (uint8_t*)(w + L.apk_inf), *hinf = (uint8_t*)(w + L.hinf), *neg_g1_inf = (uint8_t*)(w + L.neg_g1_inf), *s_inf = (uint8_t*)(w + L.s_inf);
    hipLaunchKernelGGL(k_grp_init, dim3(1), dim3(1), 0, s, flag, neg_g1, neg_g1_inf);
    GRP_CHK(c, "k_grp_init", hipGetLastError());
    // 1. the points check and KeyValidate
    if (!(flags & 1)) {                                            // ZKP_BLS_POINTS_CHECKED
        if ((rc = ctxop::valid(c, 1, pk, inf_pk, n, st, s)) || (rc = ctxop::valid(c, 2, sig, inf_sig, n, st + n, s))) return rc;
        hipLaunchKernelGGL(k_grp_fold, dim3(blocks_of(2 * n, TPB_I)), dim3(TPB_I), 0, s, (const uint8_t*)st, 2 * n, flag);
        GRP_CHK(c, "k_grp_fold", hipGetLastError());
    }
    if (inf_pk) {                                                  // the identity is no public key
        hipLaunchKernelGGL(k_grp_fold, dim3(blocks_of(n, TPB_I)), dim3(TPB_I), 0, s, (const uint8_t*)inf_pk, n, flag);
        GRP_CHK(c, "k_grp_fold", hipGetLastError());
    }
    if (com_st) {
        hipLaunchKernelGGL(k_grp_committees, dim3(blocks_of(n, TPB_I)), dim3(TPB_I), 0, s, com_st, (const uint64_t*)com_off, (uint32_t)n, flag);
        GRP_CHK(c, "k_grp_committees", hipGetLastError());
    }
    // 2. the scalars of the G2 MSM (also what flags a zero (a, b))
    hipLaunchKernelGGL(k_grp_scalars, dim3(blocks_of(n, TPB_I)), dim3(TPB_I), 0, s, (const uint64_t*)rand, n, sc, flag);
    GRP_CHK(c, "k_grp_scalars", hipGetLastError());
    // 3. A_g = sum over group g of [r_i] pk_i
    if ((rc = sums_into(c, L, w, pk, inf_pk, rand, n, grp_off, m, apk, apk_inf, (uint8_t*)(w + L.apk_st), s))) return rc;
    // 4. + 5. H_g and the Miller product of the m pairs (A_g, H_g)
    if ((rc = h2c_hash_dev(c, msgs, offsets, m, dst, dst_len, hq, hinf, s)) || (rc = ctxop::miller_product(c, apk, hq, apk_inf, hinf, m, ml, s))) return rc;
    // 6. + 7. S = sum [r_i] sig_i and the one pair (-g1, S)
    if ((rc = ctxop::msm(c, 2, sig, inf_sig, sc, n, 1, ssum, s_inf, s)) || (rc = ctxop::miller_product(c, neg_g1, ssum, neg_g1_inf, s_inf, 1, ml + 72, s))) return rc;
    // 8. + 9. one final exponentiation of the two records, then the AND
    if ((rc = ctxop::gt_is_one(c, ml, 2, ml + 72 * (grp::ML_RECORDS - 1), flag + 1, s))) return rc;
    hipLaunchKernelGGL(k_grp_finish, dim3(1), dim3(1), 0, s, (const int*)flag, (const int*)(w + L.word), all_ok);
    return ctxop::fail(c, "k_grp_finish", hipGetLastError());
}

int set_answer(zkp_ctx* c, int* all_ok, int v, hipStream_t s) {
    hipLaunchKernelGGL(k_grp_set, dim3(1), dim3(1), 0, s, all_ok, v);
    return ctxop::fail(c, "k_grp_set", hipGetLastError());
}

}  // namespace

int grp_scaled_segment_sum_dev(zkp_ctx* c, const void* pts, const void* inf, const void* rand, size_t n, const void* seg_off, size_t n_seg, void* out,
                               void* out_inf, void* status, hipStream_t s) {
    if (!n_seg && !n) return 0;
    const grp::Layout L = grp::layout(n, n_seg, false);
    void* ws = nullptr;
    if (int rc = ctxop::grow_grp(c, L.total, &ws)) return rc;
    return sums_into(c, L, (char*)ws, pts, inf, rand, n, seg_off, n_seg, (uint64_t*)out, (uint8_t*)out_inf, (uint8_t*)status, s);
}

int grp_verify_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* grp_off, const void* msgs, const void* offsets, size_t m, const void* dst,
                   size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s) {
    if (!n) return set_answer(c, all_ok, 1, s);                    // the empty batch holds, whatever m is
    const grp::Layout L = grp::layout(n, m, true);
    void* ws = nullptr;
    if (int rc = grow_all(c, n, m, 0, &ws)) return rc;
    return verify_into(c, L, (char*)ws, pk, inf_pk, grp_off, msgs, offsets, m, dst, dst_len, sig, inf_sig, n, rand, flags, nullptr, nullptr, all_ok, s);
}

int grp_fast_aggregate_verify_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* grp_off,
                                  const void* msgs, const void* offsets, size_t m, const void* dst, size_t dst_len, const void* sig, const void* inf_sig,
                                  size_t n, const void* rand, int flags, int* all_ok, hipStream_t s) {
    if (!n) return set_answer(c, all_ok, n_idx ? 0 : 1, s);        // entries and no committee to hold them: malformed by the counts alone
    const grp::Layout L = grp::layout(n, m, true);
    // the aggregates, their infinity bytes and statuses behind the verifier's regions
    const size_t apk = L.total, apk_inf = apk + msm::align256(n * 96), st = apk_inf + msm::align256(n), extra = st + msm::align256(n) - L.total;
    void* ws = nullptr;
    int rc;
    if ((rc = grow_all(c, n, m, extra, &ws))) return rc;
    char* w = (char*)ws;
    if ((rc = agg_segment_sum_dev(c, table, n_table, idx, n_idx, seg_off, n, w + apk, w + apk_inf, w + st, s))) return rc;
    return verify_into(c, L, w, w + apk, w + apk_inf, grp_off, msgs, offsets, m, dst, dst_len, sig, inf_sig, n, rand, flags, (const uint8_t*)(w + st), seg_off,
                       all_ok, s);
}

#else
}  // namespace
#endif

}  // namespace zkp
