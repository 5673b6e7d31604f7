// zkp_groth16.hip -- Fr arithmetic on the device (zkp_fr_op_batch, zkp_fr_from_wide_batch), the Fr fold (zkp_fr_fold_batch) and the
// batched Groth16 verifier (zkp_groth16_verify_batch):
//
//     prod_c e([r_c] A_c, B_c) * e(sum_c [r_c] C_c, -delta) * e(sum_i [s_i] IC_i, -gamma) * e([s_0] alpha, -beta) == 1
//     r_c = a_c + b_c z^2,   s_0 = sum_c r_c,   s_{i+1} = sum_c r_c x_{c,i}  (mod r)
//
// which is zkp_pairing_check_batch_rlc's product over the n checks e(A_c, B_c) e(-alpha, beta) e(-vk_x_c, gamma) e(-C_c, delta) with the
// vk_x column and the alpha column folded in Fr instead of summed in G1: n l Fr products and ONE MSM of l + 1 terms replace n MSMs.
//   1. points   unless ZKP_GROTH16_POINTS_CHECKED / _VK_CHECKED: is_valid of the proof / key points, statuses folded into one flag
//   2. scalars  r_c as 4-word integers; a zero (a, b) clears the flag                                   k_g16_scalars
//   3. scale    [r_c] A_c                                                                               coop_g1_mul_endo
//   4. fold     s_1 .. s_l and s_0; an input >= r clears the flag                                       k_fr_fold, k_fr_fold_finish, k_g16_place
//   5. sums     sum [r_c] C_c (one MSM of n terms); sum [s_i] IC_i and [s_0] alpha (one MSM call, two sums of l + 1 terms)
//   6. pairing  one Miller product over the n scaled pairs, one over the three folded pairs, their product, one final exponentiation
//   7. result   all_ok = (product == 1) AND the flag                                                    k_g16_finish
// The signs go onto the three fixed G2 points (k_g16_neg_g2).  Sizes come from zkp_groth16_plan.hpp; everything is queued on the
// caller's stream: no read-back, and no allocation once the workspaces have reached the call's size (capturable into a hipGraph).  The
// driver's own steps are kernel launches; the borrowed stages bring what they bring (miller_product ends in a 576-byte copy of its
// product, the MSM in its radix sort).
#include "zkp_groth16.hpp"

#include "zkp_coop.hpp"
#include "zkp_field.hpp"
#include "zkp_fr.hpp"
#include "zkp_groth16_plan.hpp"
#include "zkp_msm.hpp"
#include "zkp_rlc_plan.hpp"

namespace zkp {
namespace {

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// ------------------------------------------------------------------------------------------------------------------ Fr, one element per lane
__global__ void k_fr_check_canonical(const uint64_t* a, size_t n, int* bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t v[fr::NW];
    fr::wire_load(v, a + 4 * i);
    if (!fr::is_canonical(v)) atomicOr(bad, 1);
}
__global__ void k_fr_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x[fr::NW], y[fr::NW], r[fr::NW];
    fr::wire_load(x, a + 4 * i);
    if (op == ZKP_FR_MUL || op == ZKP_FR_ADD || op == ZKP_FR_SUB) fr::wire_load(y, b + 4 * i);
    switch (op) {
        case ZKP_FR_MUL: fr::mul(r, x, y); break;
        case ZKP_FR_ADD: fr::add(r, x, y); break;
        case ZKP_FR_SUB: fr::sub(r, x, y); break;
        case ZKP_FR_NEG: fr::neg(r, x); break;
        case ZKP_FR_SQUARE: fr::mul(r, x, x); break;
        default: fr::invert(r, x); break;
    }
    fr::wire_store(out + 4 * i, r);
}
// 64 little-endian bytes (any alignment) -> the 512-bit integer mod r
__global__ void k_fr_from_wide(const uint8_t* bytes, size_t n, uint64_t* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t v[fr::ACC_WORDS], r[fr::NW];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint8_t* p = bytes + 64 * i + 4 * k;
        v[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    v[16] = 0;
    fr::reduce_wide(r, v);
    fr::wire_store(out + 4 * i, r);
}

// ------------------------------------------------------------------------------------------------------------------ the fold
// part[(blockIdx.y l + i) 17 ..] = sum over this workgroup's rows c of w_c x_{c,i}, an exact 544-bit integer (zkp_fr.hpp, acc_mad: at
// most 2^24 products below 2^512 each, so nothing here can overflow and no reduction runs in the loop).  Lanes run along i: a thread is
// (li, rg) = (t % tw, t / tw), the workgroup covers tw consecutive i of FOLD_TPB / tw consecutive rows, so a wavefront reads contiguous
// 32-byte records of x, and strides over c with the other workgroups of its tile.  The rows of a workgroup are then joined by a tree
// over rg in LDS (word-major: lane t touches bank t % 64 only).  SUM: x = 1, i.e. the plain sum of the weights (tw = 1).
template <bool SUM>
__global__ __launch_bounds__(g16::FOLD_TPB) void k_fr_fold(const uint64_t* __restrict__ w, const uint64_t* __restrict__ x, uint32_t n, uint32_t l,
                                                           uint32_t tw_log2, uint32_t* __restrict__ part, int* ok) {
    __shared__ uint32_t sh[fr::ACC_WORDS * g16::FOLD_TPB];
    const uint32_t t = threadIdx.x, tw = 1u << tw_log2, li = t & (tw - 1), rg = t >> tw_log2, rows = g16::FOLD_TPB >> tw_log2;
    const uint32_t i = blockIdx.x * tw + li;
    uint32_t acc[fr::ACC_WORDS];
#pragma unroll
    for (int k = 0; k < fr::ACC_WORDS; k++) acc[k] = 0;
    if (SUM || i < l) {
        bool canonical = true;
        for (size_t c = (size_t)blockIdx.y * rows + rg; c < n; c += (size_t)gridDim.y * rows) {
            uint32_t ww[fr::NW];
            fr::wire_load(ww, w + 4 * c);          // 4 x u64: the ABI promises no more than the alignment of uint64_t
            if (SUM) {
                fr::acc_add(acc, ww, fr::NW);
            } else {
                uint32_t xx[fr::NW];
                fr::wire_load(xx, x + 4 * (c * l + i));
                canonical = canonical && fr::is_canonical(xx);
                fr::acc_mad(acc, ww, xx);
            }
        }
        if (ok && !canonical) ok[0] = 0;   // every writer writes the same 0: a plain store
    }
#pragma unroll
    for (int k = 0; k < fr::ACC_WORDS; k++) sh[k * g16::FOLD_TPB + t] = acc[k];
    __syncthreads();
    for (uint32_t s = rows >> 1; s >= 1; s >>= 1) {
        if (rg < s) {
            uint32_t o[fr::ACC_WORDS];
#pragma unroll
            for (int k = 0; k < fr::ACC_WORDS; k++) o[k] = sh[k * g16::FOLD_TPB + t + s * tw];
            fr::acc_add(acc, o, fr::ACC_WORDS);
#pragma unroll
            for (int k = 0; k < fr::ACC_WORDS; k++) sh[k * g16::FOLD_TPB + t] = acc[k];
        }
        __syncthreads();
    }
    if (rg == 0 && (SUM || i < l)) {
        uint32_t* dst = part + ((size_t)blockIdx.y * (SUM ? 1 : l) + (SUM ? 0 : i)) * fr::ACC_WORDS;
#pragma unroll
        for (int k = 0; k < fr::ACC_WORDS; k++) dst[k] = acc[k];
    }
}
// the second stage, a plain kernel: out[i] = (sum over the `parts` partial accumulators of i) mod r - the one reduction per output.
// g = 2^g_log2 <= 64 consecutive lanes share an output: each walks every g-th partial, a shuffle tree joins their accumulators (exact
// integers, any order), the first lane reduces.  No lane leaves before the shuffles.
__global__ __launch_bounds__(256) void k_fr_fold_finish(const uint32_t* __restrict__ part, uint32_t parts, uint32_t l, uint32_t g_log2, uint64_t* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, g = 1u << g_log2, i = t >> g_log2, sub = t & (g - 1);
    uint32_t acc[fr::ACC_WORDS];
#pragma unroll
    for (int k = 0; k < fr::ACC_WORDS; k++) acc[k] = 0;
    if (i < l)
        for (uint32_t p = sub; p < parts; p += g) {
            uint32_t o[fr::ACC_WORDS];
#pragma unroll
            for (int k = 0; k < fr::ACC_WORDS; k++) o[k] = part[((size_t)p * l + i) * fr::ACC_WORDS + k];
            fr::acc_add(acc, o, fr::ACC_WORDS);
        }
    for (uint32_t off = g >> 1; off >= 1; off >>= 1) {
        uint32_t o[fr::ACC_WORDS];
#pragma unroll
        for (int k = 0; k < fr::ACC_WORDS; k++) o[k] = __shfl_down(acc[k], off, 64);
        fr::acc_add(acc, o, fr::ACC_WORDS);
    }
    if (i < l && sub == 0) {
        uint32_t r[fr::NW];
        fr::reduce_wide(r, acc);
        fr::wire_store(out + 4 * i, r);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the verifier's small kernels
__global__ void k_g16_init(int* flag, int* all_ok, int n_zero) {
    if (n_zero) { *all_ok = 1; return; }
    flag[0] = 1;
    flag[1] = 0;
}
// any non-zero status byte clears flag[0]
__global__ void k_g16_status(const uint8_t* st, size_t n, int* flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && st[i]) flag[0] = 0;
}
// sc[4 c ..] = a_c + b_c z^2, exactly as zkp_pairing_check_batch_rlc forms it; a zero (a, b) would drop its proof: it clears flag[0]
__global__ void k_g16_scalars(const uint64_t* rand, size_t n, uint64_t* sc, int* flag) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const uint64_t a = rand[2 * c], b = rand[2 * c + 1];
    if (!a && !b) flag[0] = 0;
    uint64_t r[rlc::SCALAR_U64];
    rlc::scalar(a, b, r);
    for (size_t w = 0; w < rlc::SCALAR_U64; w++) sc[c * rlc::SCALAR_U64 + w] = r[w];
}
// dst = -src on canonical wire limbs: p - src, and 0 for 0
__device__ void wire_fp_neg(uint64_t* dst, const uint64_t* src) {
    uint32_t d[12];
    uint64_t nz = 0;
    int64_t bw = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const uint32_t v = (uint32_t)(src[i >> 1] >> (32 * (i & 1)));
        nz |= v;
        bw += (int64_t)K_P[i] - v;
        d[i] = (uint32_t)bw;
        bw >>= 32;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) dst[i] = nz ? ((uint64_t)d[2 * i] | ((uint64_t)d[2 * i + 1] << 32)) : 0;
}
// out = -delta | -gamma | -beta (x kept, both coordinates of y negated), the G2 side of the three folded pairs
__global__ void k_g16_neg_g2(const uint64_t* delta, const uint64_t* gamma, const uint64_t* beta, uint64_t* out) {
    const uint32_t t = threadIdx.x;
    if (t >= g16::FOLDED_PAIRS) return;
    const uint64_t* src = t == 0 ? delta : t == 1 ? gamma : beta;
    uint64_t* dst = out + 24 * t;
    for (int i = 0; i < 12; i++) dst[i] = src[i];
    wire_fp_neg(dst + 12, src + 12);
    wire_fp_neg(dst + 18, src + 18);
}
// the small MSM's operands, after the fold has left s_0 .. s_l in ms[0 .. l]: mp = IC_0 .. IC_l | alpha, IC_1 .. IC_l and
// ms[l + 1 ..] = s_0, 0 .. 0: one launch in place of four copies and a memset.
__global__ void k_g16_place(const uint64_t* ic, const uint64_t* alpha, uint32_t l, uint64_t* mp, uint64_t* ms) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, np = 12 * (l + 1), ns = 4 * (l + 1);
    if (i < np) {
        mp[i] = ic[i];
        mp[np + i] = i < 12 ? alpha[i] : ic[i];
    }
    if (i < ns) ms[ns + i] = i < 4 ? ms[i] : 0;
}
__global__ void k_g16_finish(const int* flag, int* all_ok) { *all_ok = (flag[0] && flag[1]) ? 1 : 0; }

// lanes per output of the second stage: the next power of two >= parts, at most a wavefront
inline uint32_t finish_lanes_log2(uint32_t parts) {
    uint32_t r = 0;
    while ((1u << r) < parts && r < 6) r++;
    return r;
}
inline uint32_t log2u(uint32_t v) {
    uint32_t r = 0;
    while ((1u << r) < v) r++;
    return r;
}

}  // namespace

hipError_t fr_check_canonical(const uint64_t* a, size_t n, int* bad, hipStream_t s) {
    hipLaunchKernelGGL(k_fr_check_canonical, dim3(blocks(n)), dim3(256), 0, s, a, n, bad);
    return hipGetLastError();
}
hipError_t fr_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_fr_op, dim3(blocks(n)), dim3(256), 0, s, op, a, b, n, out);
    return hipGetLastError();
}
hipError_t fr_from_wide(const uint8_t* bytes, size_t n, uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_fr_from_wide, dim3(blocks(n)), dim3(256), 0, s, bytes, n, out);
    return hipGetLastError();
}
hipError_t fr_fold(void* part, void* sum_part, const uint64_t* w, const uint64_t* x, size_t n, size_t l, uint64_t* out, uint64_t* sum_w, int* ok,
                   hipStream_t s) {
    const g16::FoldPlan p = g16::fold_plan(n, l);
    hipError_t e;
    if (l) {
        hipLaunchKernelGGL(k_fr_fold<false>, dim3(p.tiles, p.parts), dim3(g16::FOLD_TPB), 0, s, w, x, (uint32_t)n, (uint32_t)l, log2u(p.tw),
                           (uint32_t*)part, ok);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const uint32_t gl = finish_lanes_log2(p.parts);
        hipLaunchKernelGGL(k_fr_fold_finish, dim3(blocks(l << gl)), dim3(256), 0, s, (const uint32_t*)part, p.parts, (uint32_t)l, gl, out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (sum_w) {
        hipLaunchKernelGGL(k_fr_fold<true>, dim3(1, p.sum_parts), dim3(g16::FOLD_TPB), 0, s, w, (const uint64_t*)nullptr, (uint32_t)n, 0u, 0u,
                           (uint32_t*)sum_part, (int*)nullptr);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_fr_fold_finish, dim3(1), dim3(256), 0, s, (const uint32_t*)sum_part, p.sum_parts, 1u, finish_lanes_log2(p.sum_parts), sum_w);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

int groth16_check_dev(zkp_ctx* c, const zkp_groth16_vk* vk, const zkp_groth16_batch* b, const uint64_t* rand, int flags, int* all_ok, hipStream_t s) {
    const size_t n = b->n, l = vk->n_inputs;
    int rc;
    if (!n) {
        hipLaunchKernelGGL(k_g16_init, dim3(1), dim3(1), 0, s, (int*)nullptr, all_ok, 1);
        return ctxop::fail(c, "k_g16_init", hipGetLastError());
    }
    const g16::Layout L = g16::make_layout(n, l, flags);
    // the verifier's and the MSM's workspaces first (an allocation synchronises the device).  The stages borrowed from the context keep
    // their own grow-only buffers (miller_product's product tree, is_valid's scratch, the Miller loop's lines and state): they allocate on
    // the first call of a size and never after, which is why a call is run once before it is captured
    void* ws = nullptr;
    if ((rc = ctxop::grow_g16(c, L.total, &ws))) return rc;
    {
        const size_t b1 = msm_workspace_bytes(1, n, 1, 0), b2 = msm_workspace_bytes(1, l + 1, 2, 0);
        if ((rc = ctxop::grow_msm(c, b1 > b2 ? b1 : b2))) return rc;
    }
    char* w = (char*)ws;
    int* flag = (int*)(w + L.flag);
    uint8_t* st = (uint8_t*)(w + L.st);
    uint64_t *sc = (uint64_t*)(w + L.sc), *sg1 = (uint64_t*)(w + L.sg1), *ms = (uint64_t*)(w + L.ms), *mp = (uint64_t*)(w + L.mp);
    uint64_t *mg1 = (uint64_t*)(w + L.mg1), *mg2 = (uint64_t*)(w + L.mg2), *ml = (uint64_t*)(w + L.ml);
    uint8_t *sinf = (uint8_t*)(w + L.sinf), *minf1 = (uint8_t*)(w + L.minf1);

    hipLaunchKernelGGL(k_g16_init, dim3(1), dim3(1), 0, s, flag, all_ok, 0);
    if ((rc = ctxop::fail(c, "k_g16_init", hipGetLastError()))) return rc;
    hipLaunchKernelGGL(k_g16_neg_g2, dim3(1), dim3(64), 0, s, (const uint64_t*)vk->delta_g2, (const uint64_t*)vk->gamma_g2, (const uint64_t*)vk->beta_g2, mg2);
    if ((rc = ctxop::fail(c, "k_g16_neg_g2", hipGetLastError()))) return rc;
    // 1. the points check: the statuses side by side, then one fold (-Q is valid exactly when Q is)
    if (L.n_status) {
        uint8_t* at = st;
        auto valid = [&](int which, const void* pts, const void* inf, size_t cnt) -> int {
            const int r = ctxop::valid(c, which, pts, inf, cnt, at, s);
            at += cnt;
            return r;
        };
        if (!(flags & ZKP_GROTH16_POINTS_CHECKED) && ((rc = valid(1, b->a, b->inf_a, n)) || (rc = valid(2, b->b, b->inf_b, n)) || (rc = valid(1, b->c, b->inf_c, n))))
            return rc;
        if (!(flags & ZKP_GROTH16_VK_CHECKED) &&
            ((rc = valid(1, vk->alpha_g1, nullptr, 1)) || (rc = valid(1, vk->ic, nullptr, l + 1)) || (rc = valid(2, mg2, nullptr, g16::FOLDED_PAIRS))))
            return rc;
        hipLaunchKernelGGL(k_g16_status, dim3(blocks(L.n_status)), dim3(256), 0, s, st, L.n_status, flag);
        if ((rc = ctxop::fail(c, "k_g16_status", hipGetLastError()))) return rc;
    }
    // 2. the scalars (also what flags a zero (a, b))
    hipLaunchKernelGGL(k_g16_scalars, dim3(blocks(n)), dim3(256), 0, s, rand, n, sc, flag);
    if ((rc = ctxop::fail(c, "k_g16_scalars", hipGetLastError()))) return rc;
    // 3. + 6a. [r_c] A_c and the Miller product of the n free pairs
    if ((rc = ctxop::fail(c, "g1_mul_endo", coop_g1_mul_endo((const uint64_t*)b->a, (const uint8_t*)b->inf_a, rand, n, 1, sg1, sinf, s))) ||
        (rc = ctxop::miller_product(c, sg1, (const uint64_t*)b->b, sinf, (const uint8_t*)b->inf_b, n, ml, s)))
        return rc;
    // 4. the fold into ms[0 .. l], then the small MSM's points and the second sum's scalars: s_0 and l zeros
    if ((rc = ctxop::fail(c, "fr_fold", fr_fold(w + L.part, w + L.sum, sc, (const uint64_t*)b->inputs, n, l, ms + 4, ms, flag, s)))) return rc;
    hipLaunchKernelGGL(k_g16_place, dim3(blocks(12 * (l + 1))), dim3(256), 0, s, (const uint64_t*)vk->ic, (const uint64_t*)vk->alpha_g1, (uint32_t)l, mp, ms);
    if ((rc = ctxop::fail(c, "k_g16_place", hipGetLastError()))) return rc;
    // 5. the sums: C column; IC_0 .. IC_l and alpha, IC_1 .. IC_l (the latter under zero scalars) as two sums of one MSM call
    if ((rc = ctxop::msm(c, 1, b->c, b->inf_c, sc, n, 1, mg1, minf1, s)) || (rc = ctxop::msm(c, 1, mp, nullptr, ms, l + 1, 2, mg1 + 12, minf1 + 1, s)))
        return rc;
    // 6b. + 7. the three folded pairs, one final exponentiation of the product, then the AND
    if ((rc = ctxop::miller_product(c, mg1, mg2, minf1, nullptr, g16::FOLDED_PAIRS, ml + 72, s)) ||
        (rc = ctxop::gt_is_one(c, ml, 2, ml + 72 * (g16::ML_RECORDS - 1), flag + 1, s)))
        return rc;
    hipLaunchKernelGGL(k_g16_finish, dim3(1), dim3(1), 0, s, flag, all_ok);
    return ctxop::fail(c, "k_g16_finish", hipGetLastError());
}

}  // namespace zkp
