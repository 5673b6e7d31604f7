// zkp_bls_agg_g2.hip -- G2 segment sums on the GPU (gfx950) and the two verifiers that stand on the aggregation layer's index rules:
// zkp_g2_segment_sum_batch (signature aggregation in the min-pk layout, key aggregation in the min-sig layout),
// zkp_bls_minsig_fast_aggregate_verify_batch (committees of G2 keys) and zkp_bls_aggregate_verify_batch (min-pk AggregateVerify).
//
//   k_aggv_expand  AggregateVerify, one lane per message: the message's segment j by the bounded search of k_agg_keys; the message gets
//                  rand row j, and signature j when it is the segment's first, the flagged identity (0, 1) otherwise - into workspace rows
//   k_agg2_affine  the Jacobian G2 sums to affine wire points, ONE Fp inversion per wavefront of 64 sums (Montgomery's trick on the norms)
// The fill and the index kernels (k_agg_zero, k_agg_check, k_agg_keys, k_agg_fold) are those of zkp_bls_agg.hip, called through its aggk
// launches; between k_agg_keys and k_agg2_affine the sums are the bucket MSM's: msm_points converts the table (a G2 wire point is x.c0,
// x.c1, y.c0, y.c1: the order k_msm_accum<2, true> reads), msm_accum(2, ...) runs the levels as sums_into of zkp_bls_agg.hip drives them.
//
// tests/agg_g2_kernel_host.cpp compiles k_aggv_expand for the host (ZKP_AGG_G2_KERNELS_ONLY) under sanitizers and runs it as written on
// exactly allocated buffers.
#ifndef ZKP_AGG_G2_KERNELS_ONLY
#include "zkp_bls_agg_g2.hpp"

#include "zkp_bls.hpp"
#include "zkp_bls_agg.hpp"
#include "zkp_bls_minsig.hpp"
#include "zkp_coop.hpp"
#include "zkp_fp28_ext.hpp"
#else
#include "zkp_bls_agg_g2_plan.hpp"
#endif

namespace zkp {
namespace {

constexpr int TPB_X = 256;   // k_aggv_expand
constexpr int TPB_A2 = 64;   // k_agg2_affine: a wavefront per workgroup, the wavefront is the unit of the shared inversion

// ------------------------------------------------------------------------------------------- AggregateVerify: the expansion
// lane i < n_msg.  Sound offsets (word == 0, so n >= 1 and seg_off[0] = 0 <= i < n_msg = seg_off[n]) put message i in exactly one segment
// j: the search keeps seg_off[lo] <= i < seg_off[hi] with 0 <= lo < hi <= n, reads seg_off[1 .. n - 1] only, ends within SEARCH_STEPS and
// passes over empty segments (it finds the LAST offset at or below i).  A malformed call follows no offset and reads no signature: every
// message gets the flagged identity and the rand row (1, 0); k_agg_fold answers for it.  Reads sig[0 .. n), inf_sig[0 .. n) (may be
// null: no infinities), rand[0 .. 2 n); writes row i of the three workspace arrays.
__global__ void __launch_bounds__(TPB_X) k_aggv_expand(const uint64_t* seg_off, uint32_t n, uint32_t n_msg, const uint64_t* sig, const uint8_t* inf_sig,
                                                       const uint64_t* rand, const int* word, uint64_t* x_sig, uint8_t* x_inf, uint64_t* x_rand) {
    const uint32_t i = blockIdx.x * TPB_X + threadIdx.x;
    if (i >= n_msg) return;
    uint64_t* o = x_sig + 24 * (size_t)i;
    bool first = false;
    uint32_t lo = 0;
    if (!*word) {
        uint32_t hi = n;
        for (int step = 0; step < agg::SEARCH_STEPS && hi - lo > 1; step++) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (seg_off[mid] <= i) lo = mid; else hi = mid;
        }
        first = seg_off[lo] == i;
        x_rand[2 * (size_t)i] = rand[2 * (size_t)lo];
        x_rand[2 * (size_t)i + 1] = rand[2 * (size_t)lo + 1];
    } else {
        x_rand[2 * (size_t)i] = 1;
        x_rand[2 * (size_t)i + 1] = 0;
    }
    if (first) {
        const uint64_t* s = sig + 24 * (size_t)lo;
        for (int k = 0; k < 24; k++) o[k] = s[k];
        x_inf[i] = inf_sig ? inf_sig[lo] : 0;
    } else {
        for (int k = 0; k < 24; k++) o[k] = k == 12 ? 1 : 0;
        x_inf[i] = 1;
    }
}

#ifndef ZKP_AGG_G2_KERNELS_ONLY
using zkp28::Fp28;
using zkp28::NL;
using namespace zkp_f28;

// ------------------------------------------------------------------------------------------- Jacobian G2 sums -> affine wire points
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

// One lane per sum, a wavefront per workgroup (the other form, two lanes per sum with the F2 policy of zkp_coop.hip, would share one
// inversion among 32 sums only and needs that file's by-value field routines; this form is k_agg_affine with an Fp2 tail).  A sum is six
// records: x.c0, x.c1, y.c0, y.c1, z.c0, z.c1.  The norm N = z0^2 + z1^2 of Z = z0 + z1 u lies in Fp and vanishes only for Z = 0 (p = 3
// mod 4: -1 is no square), so the chain of k_agg_affine - inclusive prefix and suffix products across the 64 lanes through LDS, ONE
// inversion of the wavefront's product - runs over the norms: 1 / N_l = P_(l-1) S_(l+1) / P_63.  Then 1 / Z = conj(Z) / N, and Z^-2,
// Z^-3 in Fp2; Z, X and Y are reloaded from the records where they are used rather than kept live across the chain.  A sum at infinity
// (both coefficients of Z zero: the stored limbs are not canonical, the test canonicalises each), a sum whose status is set and every sum
// of a malformed call enter the chain as 1 and come out as the identity (0, 1) with out_inf = 1, so the shared product is never zero.
// Per lane 2 products of norm, 12 + 2 of the chain, 2 of the conjugate, 2 + 4 + 4 + 4 of the Fp2 tail, beside the wavefront's 461; the
// wire words are the canonical values of X / Z^2 and Y / Z^3.  The final status is written here: status | word.
__global__ void __launch_bounds__(TPB_A2) k_agg2_affine(const int4* sums, uint32_t n_seg, const int* word, uint8_t* status, uint64_t* out, uint8_t* out_inf) {
    __shared__ int4 sh[2 * 4 * 64];
    const int lane = threadIdx.x;
    const uint32_t j = blockIdx.x * TPB_A2 + lane;
    const bool live = j < n_seg;
    const uint32_t jj = live ? j : n_seg - 1;
    const int4* rec = sums + (size_t)jj * 24;
    const bool refused = *word || (live && status[j]);
    Fp28 one, nrm;
    f_const(one, zkp28::K28_ONE);
    bool dead;
    {
        Fp28 z0, z1;
        rec_ld(z0, rec + 16);
        rec_ld(z1, rec + 20);
        const bool z0_zero = f_is_zero(z0), z1_zero = f_is_zero(z1);
        dead = !live || refused || (z0_zero && z1_zero);
        f_mul2(nrm, z0, z0, z1, z1);
    }
    f_pick(nrm, one, dead);
    Fp28 pre = nrm, suf = nrm;
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
    Fp28 total, before = one, after = one, ni, t;
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
    f_mul(ni, before, t);                     // 1 / N
    F2 zi, zi2, p, ax, ay;
    rec_ld(t, rec + 16);
    f_mul(zi.c0, t, ni);
    rec_ld(t, rec + 20);
    f_neg(t, t);                              // the conjugate
    f_mul(zi.c1, t, ni);
    f2_sqr(zi2, zi);
    rec_ld(p.c0, rec);
    rec_ld(p.c1, rec + 4);
    f2_mul(ax, p, zi2);
    f2_mul(zi2, zi2, zi);
    rec_ld(p.c0, rec + 8);
    rec_ld(p.c1, rec + 12);
    f2_mul(ay, p, zi2);
    if (!live) return;
    uint64_t* o = out + 24 * (size_t)j;
    uint64_t w[6];
    zkp28::fp28_to_wire(w, ax.c0);
#pragma unroll
    for (int k = 0; k < 6; k++) o[k] = dead ? 0 : w[k];
    zkp28::fp28_to_wire(w, ax.c1);
#pragma unroll
    for (int k = 0; k < 6; k++) o[6 + k] = dead ? 0 : w[k];
    zkp28::fp28_to_wire(w, ay.c0);
#pragma unroll
    for (int k = 0; k < 6; k++) o[12 + k] = dead ? (k == 0 ? 1 : 0) : w[k];
    zkp28::fp28_to_wire(w, ay.c1);
#pragma unroll
    for (int k = 0; k < 6; k++) o[18 + k] = dead ? 0 : w[k];
    out_inf[j] = dead ? 1 : 0;
    status[j] = refused ? 1 : 0;
}

inline unsigned blocks_of(size_t n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

#define AGG2_CHK(c, what, call)                                       \
    do {                                                              \
        if (int rc__ = ctxop::fail((c), (what), (call))) return rc__; \
    } while (0)

// the six steps of sums_into (zkp_bls_agg.hip) on a workspace of layout L, with G2 records; out / out_inf / status: device, n_seg rows
int sums_into(zkp_ctx* c, const agg2::Layout& L, char* w, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg,
              uint64_t* out, uint8_t* out_inf, uint8_t* status, hipStream_t s) {
    int* word = (int*)(w + L.word);
    uint32_t *keys = (uint32_t*)(w + L.keys), *vals = (uint32_t*)(w + L.vals);
    uint32_t* part_k[2] = {(uint32_t*)(w + L.part_k[0]), (uint32_t*)(w + L.part_k[1])};
    void* part_j[2] = {w + L.part_j[0], w + L.part_j[1]};
    int rc;
    AGG2_CHK(c, "k_msm_points", msm_points((const uint64_t*)table, (uint32_t)(4 * n_table), w + L.pts, s));
    // the word and the sums in one fill, before the check that may set the word
    if ((rc = aggk::zero(c, word, L.fill, s)) || (rc = aggk::check(c, seg_off, n_seg, n_idx, status, word, s)) ||
        (rc = aggk::keys(c, idx, n_idx, seg_off, n_seg, n_table, word, keys, vals, status, s)))
        return rc;
    // level 0 from the entries, then the partial sums ping-pong until one run is left (msm_run's loop)
    uint32_t n = (uint32_t)n_idx;
    const uint32_t* kin = keys;
    const void* jin = w + L.pts;
    for (int lv = 0; n; lv++) {
        AGG2_CHK(c, "k_msm_accum", msm_accum(2, lv == 0, kin, vals, jin, n, (uint32_t)n_seg, w + L.sums, part_k[lv & 1], part_j[lv & 1], s));
        if (n <= msm::RUN) break;
        n = 2 * msm::runs_of(n);
        kin = part_k[lv & 1];
        jin = part_j[lv & 1];
    }
    if (n_seg) {
        hipLaunchKernelGGL(k_agg2_affine, dim3(blocks_of(n_seg, TPB_A2)), dim3(TPB_A2), 0, s, (const int4*)(w + L.sums), (uint32_t)n_seg, (const int*)word, status,
                           out, out_inf);
        AGG2_CHK(c, "k_agg2_affine", hipGetLastError());
    }
    return 0;
}

}  // namespace

int agg2_segment_sum_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, void* out,
                         void* out_inf, void* status, hipStream_t s) {
    if (!n_seg && !n_idx) return 0;
    const agg2::Layout L = agg2::layout(n_table, n_idx, n_seg, false);
    void* ws = nullptr;
    if (int rc = ctxop::grow_agg(c, L.total, &ws)) return rc;
    return sums_into(c, L, (char*)ws, table, n_table, idx, n_idx, seg_off, n_seg, (uint64_t*)out, (uint8_t*)out_inf, (uint8_t*)status, s);
}

int agg2_minsig_verify_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* msgs,
                           const void* offsets, const void* dst, size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags,
                           int* all_ok, hipStream_t s) {
    if (!n && !n_idx) return minsig_verify_dev(c, nullptr, nullptr, msgs, offsets, dst, dst_len, sig, inf_sig, 0, rand, flags, all_ok, s);   // the empty batch holds
    const agg2::Layout L = agg2::layout(n_table, n_idx, n, true);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_agg(c, L.total, &ws))) return rc;
    char* w = (char*)ws;
    uint64_t* apk = (uint64_t*)(w + L.apk);
    uint8_t *apk_inf = (uint8_t*)(w + L.apk_inf), *st = (uint8_t*)(w + L.st);
    // the sums (with n = 0 still the check of the offsets: a call of no committee and some entries is malformed)
    if ((rc = sums_into(c, L, w, table, n_table, idx, n_idx, seg_off, n, apk, apk_inf, st, s))) return rc;
    if ((rc = minsig_verify_dev(c, apk, apk_inf, msgs, offsets, dst, dst_len, sig, inf_sig, n, rand, flags, all_ok, s))) return rc;
    return aggk::fold(c, st, seg_off, n, (const int*)(w + L.word), all_ok, s);
}

int aggv_verify_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* msgs, const void* offsets, size_t n_msg, const void* seg_off, const void* dst,
                    size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s) {
    if (!n && !n_msg) return bls_verify_dev(c, nullptr, nullptr, msgs, offsets, dst, dst_len, nullptr, nullptr, 0, rand, flags, all_ok, s);   // the empty batch holds
    const agg2::Expand L = agg2::expand_layout(n_msg, n);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_agg(c, L.total, &ws))) return rc;
    char* w = (char*)ws;
    int* word = (int*)(w + L.word);
    uint8_t* st = (uint8_t*)(w + L.st);
    uint64_t *x_sig = (uint64_t*)(w + L.sig), *x_rand = (uint64_t*)(w + L.rand);
    uint8_t* x_inf = (uint8_t*)(w + L.inf_sig);
    // the offsets are checked as a committee's: from 0 to n_msg, non-decreasing (with n = 0 and messages: malformed)
    if ((rc = aggk::zero(c, word, 256, s)) || (rc = aggk::check(c, seg_off, n, n_msg, st, word, s))) return rc;
    if (n_msg) {
        hipLaunchKernelGGL(k_aggv_expand, dim3(blocks_of(n_msg, TPB_X)), dim3(TPB_X), 0, s, (const uint64_t*)seg_off, (uint32_t)n, (uint32_t)n_msg,
                           (const uint64_t*)sig, (const uint8_t*)inf_sig, (const uint64_t*)rand, (const int*)word, x_sig, x_inf, x_rand);
        AGG2_CHK(c, "k_aggv_expand", hipGetLastError());
    }
    if ((rc = bls_verify_dev(c, pk, inf_pk, msgs, offsets, dst, dst_len, x_sig, x_inf, n_msg, x_rand, flags, all_ok, s))) return rc;
    // an empty segment (a signature over no pair) or a malformed call stores 0
    return aggk::fold(c, st, seg_off, n, word, all_ok, s);
}

#else
}  // namespace
#endif

}  // namespace zkp
