// zkp_kzg.hip -- the batched Fr inversion (zkp_fr_invert_batch), the barycentric evaluation of polynomials held in evaluation form
// (zkp_fr_eval_batch) and the batch KZG opening verifier (zkp_kzg_verify_batch).
//
// Inversion, Montgomery's trick on three levels (zkp_fr.hpp: the per-thread pieces and why canonical elements can be multiplied as they
// come; zkp_kzg_plan.hpp: the sizes):
//   up     a thread owns INV_RUN = 4 consecutive elements (zeros replaced by one) and multiplies them up; a tree over LDS joins the 256
//          run totals of the workgroup into one 32-byte total                                                      k_frinv_up
//   mid    ONE workgroup: each thread a run of consecutive workgroup totals, prefix products kept beside them, the run totals scanned
//          over LDS (prefix and suffix), ONE power r - 2 of the grand total, the back-sweep over the totals          k_frinv_mid
//   down   the runs and the two LDS scans again, the inverse of the thread's run total = (product of the other run totals) x (inverse
//          of the workgroup total), the back-sweep over the run, zeros written back as zeros                        k_frinv_down
// Products per call, counted (tests/test_kzg_cpu.py runs the same schedule on the host and counts): a full workgroup of 1024 elements
// performs 768 + 255 (up) and 768 + 3586 + 510 + 1536 (down) = 7423, i.e. 7.25 per element; the middle launch adds three per 1024 and
// one power r - 2 per CALL.  Lanes beyond the data perform nothing, so a short tail stays below 8 per element as well.  No atomics; exact
// arithmetic, so the result does not depend on the grid.
//
// Evaluation: y = (z^N - 1) / N * sum_i f_i w^i / (z - w^i) over the domain w^i = omega_k^i, composed: denominators (k_freval_den),
// the inversion above in place, then the sum (k_freval_sum: min(N, 256) lanes per polynomial, modular adds, a tree over LDS).  A zero
// denominator - found as a zero "inverse" - means z = w^i and y = f_i.
//
// Verifier: n openings (C_i, z_i, y_i, pi_i) of one setup (g1, g2, [tau]g2); opening i holds iff
// e(C_i - [y_i]g1 + [z_i]pi_i, g2) = e(pi_i, [tau]g2).  With r_i = a_i + b_i z^2 (zkp_rlc_plan.hpp), t_i = r_i z_i, u = sum r_i y_i:
//     e(sum r_i C_i + sum t_i pi_i - [u]g1, -g2) * e(sum r_i pi_i, [tau]g2) == 1
//   1. points   unless ZKP_KZG_POINTS_CHECKED / _VK_CHECKED: is_valid of C, pi / g1, -g2, [tau]g2, statuses folded into one flag
//   2. scalars  r_i, t_i; a zero (a, b) or a z_i >= r clears the flag                                  k_kzg_scalars
//   3. fold     u by fr_fold with l = 1; a y_i >= r clears the flag                                     (zkp_groth16.hip)
//   4. place    points C | pi | g1 and the scalar -u behind r | t                                       k_kzg_place
//   5. sums     ONE shared-bases MSM call over the 2 n + 1 points: row 0 = r | t | -u, row 1 = 0 | r | 0 (the zeros cost less than a
//               second call's fixed latency).  Where 2 (2 n + 1) terms exceed the MSM's limit - n = 2^22 alone - two
//               calls: row 0, then the caller's pi under the r_i of row 0
//   6. pairing  one Miller product over the two pairs, one final exponentiation, == 1
//   7. result   all_ok = (product == 1) AND the flag                                                    k_kzg_finish
// Everything is queued on the caller's stream: no read-back, and no allocation once the workspaces have reached the call's size.
#include "zkp_kzg.hpp"

#include "zkp_field.hpp"
#include "zkp_fr.hpp"
#include "zkp_groth16_plan.hpp"
#include "zkp_kzg_plan.hpp"
#include "zkp_msm.hpp"
#include "zkp_msm_plan.hpp"
#include "zkp_rlc_plan.hpp"

namespace zkp {
namespace {

using fr::NW;
constexpr int TPB = fr::INV_TPB, RUN = fr::INV_RUN;
static_assert((size_t)fr::INV_RUN == kzg::INV_RUN && (size_t)fr::INV_TPB == kzg::INV_TPB, "zkp_fr.hpp and zkp_kzg_plan.hpp agree");
constexpr fr::Roots ROOTS = fr::make_roots();   // host side: the launches pass the elements they need by value

struct FrWords { uint32_t w[NW]; };
inline FrWords words_of(const uint32_t* v) {
    FrWords f;
    for (int i = 0; i < NW; i++) f.w[i] = v[i];
    return f;
}
inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// LDS is word-major: lane t touches bank t % 64 only
__device__ __forceinline__ void sh_put(uint32_t* sh, uint32_t t, const uint32_t* v) {
#pragma unroll
    for (int k = 0; k < NW; k++) sh[k * TPB + t] = v[k];
}
__device__ __forceinline__ void sh_get(uint32_t* v, const uint32_t* sh, uint32_t t) {
#pragma unroll
    for (int k = 0; k < NW; k++) v[k] = sh[k * TPB + t];
}
__device__ __forceinline__ void copy8(uint32_t* d, const uint32_t* s) {
#pragma unroll
    for (int k = 0; k < NW; k++) d[k] = s[k];
}

// ------------------------------------------------------------------------------------------------------------------ the inversion
// the thread's run: elements first .. first + m - 1 of a (4 x u64 each: the ABI promises no more than the alignment of uint64_t)
__device__ __forceinline__ int run_load(const uint64_t* __restrict__ a, size_t n, size_t first, fr::InvRun& r) {
    const int m = first < n ? (n - first < (size_t)RUN ? (int)(n - first) : RUN) : 0;
    if (m > 0) fr::wire_load(r.x0, a + 4 * first);
    if (m > 1) fr::wire_load(r.x1, a + 4 * (first + 1));
    if (m > 2) fr::wire_load(r.x2, a + 4 * (first + 2));
    if (m > 3) fr::wire_load(r.x3, a + 4 * (first + 3));
    return m;
}
// threads of this workgroup that hold data
__device__ __forceinline__ uint32_t active_threads(size_t n, size_t base) {
    const size_t left = n - base;
    return left >= (size_t)fr::INV_BLOCK ? (uint32_t)TPB : (uint32_t)((left + RUN - 1) / RUN);
}
// oth = the product of the totals T of the OTHER threads below na (false: there is none), by an inclusive prefix scan P and an
// inclusive suffix scan Q over LDS (sh: 2 x NW x TPB words); P[na - 1] is the workgroup's total afterwards.  Threads at or above na
// multiply nothing.
__device__ __forceinline__ bool wg_others(uint32_t* sh, uint32_t t, uint32_t na, const uint32_t* T, uint32_t* oth) {
    uint32_t *P = sh, *Q = sh + NW * TPB;
    uint32_t pp[NW], qq[NW];
    copy8(pp, T);
    copy8(qq, T);
    sh_put(P, t, pp);
    sh_put(Q, t, qq);
    __syncthreads();
    for (uint32_t d = 1; d < na; d <<= 1) {
        const bool dp = t >= d && t < na, dq = t + d < na;
        uint32_t o1[NW], o2[NW];
        if (dp) sh_get(o1, P, t - d);
        if (dq) sh_get(o2, Q, t + d);
        __syncthreads();
        if (dp) {
            fr::mont_mul(pp, pp, o1);
            sh_put(P, t, pp);
        }
        if (dq) {
            fr::mont_mul(qq, qq, o2);
            sh_put(Q, t, qq);
        }
        __syncthreads();
    }
    bool any = false;
    if (t < na) {
        if (t > 0) {
            sh_get(oth, P, t - 1);
            any = true;
        }
        if (t + 1 < na) {
            uint32_t s2[NW];
            sh_get(s2, Q, t + 1);
            if (any) fr::mont_mul(oth, oth, s2);
            else copy8(oth, s2);
            any = true;
        }
    }
    return any;
}

__global__ __launch_bounds__(TPB) void k_frinv_up(const uint64_t* __restrict__ a, size_t n, uint32_t* __restrict__ tot) {
    __shared__ uint32_t sh[NW * TPB];
    const uint32_t t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * fr::INV_BLOCK;
    const uint32_t na = active_threads(n, base);
    fr::InvRun r;
    uint32_t T[NW], zm;
    const int m = run_load(a, n, base + (size_t)t * RUN, r);
    fr::inv_run_prefix(r, T, &zm, m);
    sh_put(sh, t, T);
    __syncthreads();
    for (uint32_t s = TPB / 2; s >= 1; s >>= 1) {
        if (t < s && t + s < na) {
            uint32_t o[NW];
            sh_get(o, sh, t + s);
            fr::mont_mul(T, T, o);
            sh_put(sh, t, T);
        }
        __syncthreads();
    }
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < NW; k++) tot[(size_t)blockIdx.x * NW + k] = T[k];
    }
}
// one workgroup over the nb workgroup totals: thread t owns totals t run .. t run + run - 1; na = the threads that own any.  tot[j] is
// replaced by the inverse of total j, scaled by rinv (zkp_fr.hpp) so that the elements below come out canonical.
__global__ __launch_bounds__(TPB) void k_frinv_mid(uint32_t* __restrict__ tot, uint32_t* __restrict__ pre, uint32_t nb, uint32_t run, uint32_t na) {
    __shared__ uint32_t sh[2 * NW * TPB];
    __shared__ uint32_t top[NW];
    constexpr fr::Consts K = fr::make_consts();
    constexpr fr::Roots W = fr::make_roots();
    const uint32_t t = threadIdx.x;
    const uint32_t lo = t < na ? t * run : nb, hi = t < na ? (nb - lo < run ? nb : lo + run) : nb;
    uint32_t T[NW];
    copy8(T, K.one);
    for (uint32_t j = lo; j < hi; j++) {
        uint32_t v[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) v[k] = tot[(size_t)j * NW + k];
        if (j == lo) copy8(T, v);
        else fr::mont_mul(T, T, v);
#pragma unroll
        for (int k = 0; k < NW; k++) pre[(size_t)j * NW + k] = T[k];
    }
    uint32_t u[NW];
    const bool any = wg_others(sh, t, na, T, u);
    if (t == 0) {
        uint32_t g[NW];
        sh_get(g, sh, na - 1);
        fr::mont_inv(g, g);
        fr::mont_mul(g, g, W.rinv);
#pragma unroll
        for (int k = 0; k < NW; k++) top[k] = g[k];
    }
    __syncthreads();
    if (t >= na) return;
    uint32_t g[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) g[k] = top[k];
    if (any) fr::mont_mul(u, u, g);
    else copy8(u, g);
    for (uint32_t j = hi; j-- > lo + 1;) {
        uint32_t v[NW], q[NW], o[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) {
            v[k] = tot[(size_t)j * NW + k];
            q[k] = pre[(size_t)(j - 1) * NW + k];
        }
        fr::mont_mul(o, u, q);
        fr::mont_mul(u, u, v);
#pragma unroll
        for (int k = 0; k < NW; k++) tot[(size_t)j * NW + k] = o[k];
    }
#pragma unroll
    for (int k = 0; k < NW; k++) tot[(size_t)lo * NW + k] = u[k];
}
__global__ __launch_bounds__(TPB) void k_frinv_down(const uint64_t* a, size_t n, const uint32_t* __restrict__ tot, uint64_t* out) {
    __shared__ uint32_t sh[2 * NW * TPB];
    const uint32_t t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * fr::INV_BLOCK, first = base + (size_t)t * RUN;
    const uint32_t na = active_threads(n, base);
    fr::InvRun r;
    uint32_t T[NW], zm;
    const int m = run_load(a, n, first, r);
    fr::inv_run_prefix(r, T, &zm, m);
    uint32_t u[NW];
    const bool any = wg_others(sh, t, na, T, u);
    if (t >= na) return;
    uint32_t g[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) g[k] = tot[(size_t)blockIdx.x * NW + k];
    if (any) fr::mont_mul(u, u, g);
    else copy8(u, g);
    fr::inv_run_back(r, u, zm, m);
    if (m > 0) fr::wire_store(out + 4 * first, r.x0);
    if (m > 1) fr::wire_store(out + 4 * (first + 1), r.p1);
    if (m > 2) fr::wire_store(out + 4 * (first + 2), r.p2);
    if (m > 3) fr::wire_store(out + 4 * (first + 3), r.p3);
}

// ------------------------------------------------------------------------------------------------------------------ the evaluation
// table[i] = w^i in Montgomery form, i < n, by the bits of i
__global__ void k_freval_domain(uint32_t* table, uint32_t n, FrWords w) {
    constexpr fr::Consts K = fr::make_consts();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t res[NW], b[NW];
    copy8(res, K.one);
    copy8(b, w.w);
#pragma unroll 1
    for (uint32_t e = i; e; e >>= 1) {
        if (e & 1) fr::mont_mul(res, res, b);
        fr::mont_mul(b, b, b);
    }
#pragma unroll
    for (int k = 0; k < NW; k++) table[(size_t)i * NW + k] = res[k];
}
// the domain index of evaluation i: i itself, or its k-bit reversal
__device__ __forceinline__ uint32_t domain_index(uint32_t i, uint32_t k, int bitrev) { return (bitrev && k) ? __brev(i) >> (32 - k) : i; }
// den[j N + i] = z_j - w^idx(i), canonical
__global__ void k_freval_den(const uint64_t* __restrict__ z, const uint32_t* __restrict__ table, uint32_t tshift, uint32_t k, int bitrev, uint32_t total,
                              uint64_t* __restrict__ den) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint32_t i = e & ((1u << k) - 1), j = e >> k;
    const size_t at = (size_t)domain_index(i, k, bitrev) << tshift;
    uint32_t w[NW], zz[NW], d[NW];
#pragma unroll
    for (int q = 0; q < NW; q++) w[q] = table[at * NW + q];
    fr::from_mont(w, w);
    fr::wire_load(zz, z + 4 * (size_t)j);
    fr::sub(d, zz, w);
    fr::wire_store(den + 4 * (size_t)e, d);
}
// out[j] = (z_j^N - 1) / N * sum_i f_{j,i} w^idx(i) dinv_{j,i}, or f_{j,i} where dinv_{j,i} = 0 (z_j = w^idx(i): at most one i).
// 2^tp_log2 = min(N, 256) lanes share a polynomial, 256 >> tp_log2 polynomials a workgroup.
__global__ __launch_bounds__(TPB) void k_freval_sum(const uint64_t* __restrict__ evals, const uint64_t* __restrict__ z, const uint64_t* __restrict__ dinv,
                                                     const uint32_t* __restrict__ table, uint32_t tshift, uint32_t k, int bitrev, uint32_t n_poly,
                                                     uint32_t tp_log2, FrWords ninv, uint64_t* __restrict__ out) {
    __shared__ uint32_t sh[NW * TPB];
    __shared__ uint32_t hit[TPB];
    constexpr fr::Consts K = fr::make_consts();
    const uint32_t t = threadIdx.x, tp = 1u << tp_log2, li = t & (tp - 1), pg = t >> tp_log2, n_ev = 1u << k;
    const uint32_t j = blockIdx.x * (TPB >> tp_log2) + pg;
    if (li == 0) hit[pg] = 0;
    __syncthreads();
    uint32_t acc[NW];
#pragma unroll
    for (int q = 0; q < NW; q++) acc[q] = 0;
    if (j < n_poly) {
        for (uint32_t i = li; i < n_ev; i += tp) {
            const size_t e = ((size_t)j << k) + i;
            uint32_t di[NW], f[NW], w[NW], nz = 0;
            fr::wire_load(di, dinv + 4 * e);
#pragma unroll
            for (int q = 0; q < NW; q++) nz |= di[q];
            if (!nz) {
                hit[pg] = i + 1;   // one writer per polynomial: the w^i are distinct
                continue;
            }
            fr::wire_load(f, evals + 4 * e);
            const size_t at = (size_t)domain_index(i, k, bitrev) << tshift;
#pragma unroll
            for (int q = 0; q < NW; q++) w[q] = table[at * NW + q];
            fr::mont_mul(f, f, w);     // f w
            fr::mont_mul(f, f, di);    // f w / (z - w) / R
            fr::add(acc, acc, f);
        }
    }
    sh_put(sh, t, acc);
    __syncthreads();
    for (uint32_t s = tp >> 1; s >= 1; s >>= 1) {
        if (li < s) {
            uint32_t o[NW];
            sh_get(o, sh, t + s);
            fr::add(acc, acc, o);
            sh_put(sh, t, acc);
        }
        __syncthreads();
    }
    if (li != 0 || j >= n_poly) return;
    uint64_t* dst = out + 4 * (size_t)j;
    if (hit[pg]) {
        const uint64_t* src = evals + 4 * (((size_t)j << k) + hit[pg] - 1);
        for (int q = 0; q < 4; q++) dst[q] = src[q];
        return;
    }
    uint32_t zz[NW], y[NW];
    fr::wire_load(zz, z + 4 * (size_t)j);
    fr::to_mont(zz, zz);
#pragma unroll 1
    for (uint32_t q = 0; q < k; q++) fr::mont_mul(zz, zz, zz);   // z^N R
    fr::sub(zz, zz, K.one);                                      // (z^N - 1) R
    fr::mont_mul(zz, zz, ninv.w);                                // (z^N - 1) / N R
    fr::mont_mul(zz, zz, K.r2);                                  // ... R^2
    fr::mont_mul(y, acc, zz);                                    // (sum / R) (z^N - 1) / N R^2 / R
    fr::wire_store(dst, y);
}

// ------------------------------------------------------------------------------------------------------------------ the verifier's small kernels
__global__ void k_kzg_init(int* flag, int* all_ok, int n_zero) {
    if (n_zero) { *all_ok = 1; return; }
    flag[0] = 1;
    flag[1] = 0;
}
// any non-zero status byte clears flag[0]
__global__ void k_kzg_status(const uint8_t* st, size_t n, int* flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && st[i]) flag[0] = 0;   // every writer writes the same 0: a plain store
}
// ms[i] = r_i = a_i + b_i z^2 exactly as zkp_pairing_check_batch_rlc forms it, ms[n + i] = t_i = r_i z_i mod r; a zero (a, b) would drop its
// opening and z_i + r is not z_i to a verifier: both clear flag[0].  row1 (null for the two-call path): the second row 0 | r | 0
__global__ void k_kzg_scalars(const uint64_t* rand, const uint64_t* z, size_t n, uint64_t* ms, uint64_t* row1, int* flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = rand[2 * i], b = rand[2 * i + 1];
    uint64_t r[rlc::SCALAR_U64];
    rlc::scalar(a, b, r);
    uint32_t rw[NW], zw[NW], tw[NW];
    fr::wire_load(rw, r);
    fr::wire_load(zw, z + 4 * i);
    if ((!a && !b) || !fr::is_canonical(zw)) flag[0] = 0;
    fr::mul(tw, zw, rw);
    for (size_t w = 0; w < rlc::SCALAR_U64; w++) ms[4 * i + w] = r[w];
    fr::wire_store(ms + 4 * (n + i), tw);
    if (row1)
        for (size_t w = 0; w < rlc::SCALAR_U64; w++) {
            row1[4 * i + w] = 0;
            row1[4 * (n + i) + w] = r[w];
        }
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
// out = -g2 | [tau]g2, the G2 side of the two pairs
__global__ void k_kzg_g2(const uint64_t* g2, const uint64_t* tau_g2, uint64_t* out) {
    if (threadIdx.x == 0) {
        for (int i = 0; i < 12; i++) out[i] = g2[i];
        wire_fp_neg(out + 12, g2 + 12);
        wire_fp_neg(out + 18, g2 + 18);
    } else if (threadIdx.x == 1) {
        for (int i = 0; i < 24; i++) out[24 + i] = tau_g2[i];
    }
}
// the MSM's operands behind the scalars r | t: points C | pi | g1 with their infinity bytes, the scalar -u, and row 1's last 0
__global__ void k_kzg_place(const uint64_t* cp, const uint8_t* cinf, const uint64_t* pp, const uint8_t* pinf, const uint64_t* g1, const uint64_t* u,
                            size_t n, uint64_t* mp, uint8_t* minf, uint64_t* ms, uint64_t* row1) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 12 * n) mp[i] = cp[i];
    else if (i < 24 * n) mp[i] = pp[i - 12 * n];
    else if (i < 24 * n + 12) mp[i] = g1[i - 24 * n];
    if (i < n) minf[i] = cinf ? cinf[i] : 0;
    else if (i < 2 * n) minf[i] = pinf ? pinf[i - n] : 0;
    else if (i == 2 * n) minf[i] = 0;
    if (i == 0) {
        uint32_t uw[NW];
        fr::wire_load(uw, u);
        fr::neg(uw, uw);
        fr::wire_store(ms + 4 * 2 * n, uw);
        if (row1)
            for (int w = 0; w < 4; w++) row1[4 * 2 * n + w] = 0;
    }
}
__global__ void k_kzg_finish(const int* flag, int* all_ok) { *all_ok = (flag[0] && flag[1]) ? 1 : 0; }

}  // namespace

hipError_t fr_domain_build(uint32_t* table, unsigned log2_n, hipStream_t s) {
    const uint32_t n = 1u << log2_n;
    hipLaunchKernelGGL(k_freval_domain, dim3(blocks(n)), dim3(256), 0, s, table, n, words_of(ROOTS.omega[log2_n]));
    return hipGetLastError();
}
hipError_t fr_invert(void* ws, const uint64_t* a, size_t n, uint64_t* out, hipStream_t s) {
    const kzg::InvPlan p = kzg::inv_plan(n);
    uint32_t *tot = (uint32_t*)((char*)ws + p.tot), *pre = (uint32_t*)((char*)ws + p.pre);
    hipError_t e;
    hipLaunchKernelGGL(k_frinv_up, dim3((unsigned)p.blocks), dim3(TPB), 0, s, a, n, tot);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_frinv_mid, dim3(1), dim3(TPB), 0, s, tot, pre, (uint32_t)p.blocks, (uint32_t)p.mid_run, (uint32_t)p.mid_threads);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_frinv_down, dim3((unsigned)p.blocks), dim3(TPB), 0, s, a, n, (const uint32_t*)tot, out);
    return hipGetLastError();
}
hipError_t fr_eval(void* ws, const uint32_t* table, unsigned table_log2, const uint64_t* evals, const uint64_t* z, size_t n_poly, unsigned log2_n, int flags,
                   uint64_t* out, hipStream_t s) {
    const kzg::EvalLayout L = kzg::eval_layout(n_poly, log2_n);
    const size_t total = n_poly << log2_n;
    const int bitrev = (flags & ZKP_FR_EVAL_BITREV) ? 1 : 0;
    const uint32_t tshift = table_log2 - log2_n;
    uint64_t* den = (uint64_t*)((char*)ws + L.den);
    hipError_t e;
    hipLaunchKernelGGL(k_freval_den, dim3(blocks(total)), dim3(256), 0, s, z, table, tshift, (uint32_t)log2_n, bitrev, (uint32_t)total, den);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = fr_invert(ws, den, total, den, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_freval_sum, dim3((unsigned)L.sum_blocks), dim3(TPB), 0, s, evals, z, (const uint64_t*)den, table, tshift, (uint32_t)log2_n, bitrev,
                       (uint32_t)n_poly, (uint32_t)L.tp_log2, words_of(ROOTS.inv_pow2[log2_n]), out);
    return hipGetLastError();
}

hipError_t kzg_flag_init(int* flag, int* all_ok, int n_zero, hipStream_t s) {
    hipLaunchKernelGGL(k_kzg_init, dim3(1), dim3(1), 0, s, flag, all_ok, n_zero);
    return hipGetLastError();
}
hipError_t kzg_flag_status(const uint8_t* st, size_t n, int* flag, hipStream_t s) {
    hipLaunchKernelGGL(k_kzg_status, dim3(blocks(n)), dim3(256), 0, s, st, n, flag);
    return hipGetLastError();
}
hipError_t kzg_g2_side(const uint64_t* g2, const uint64_t* tau_g2, uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_kzg_g2, dim3(1), dim3(64), 0, s, g2, tau_g2, out);
    return hipGetLastError();
}
hipError_t kzg_flag_finish(const int* flag, int* all_ok, hipStream_t s) {
    hipLaunchKernelGGL(k_kzg_finish, dim3(1), dim3(1), 0, s, flag, all_ok);
    return hipGetLastError();
}

int kzg_check_dev(zkp_ctx* c, const zkp_kzg_vk* vk, const zkp_kzg_batch* b, const uint64_t* rand, int flags, int* all_ok, hipStream_t s) {
    const size_t n = b->n;
    int rc;
    if (!n) {
        hipLaunchKernelGGL(k_kzg_init, dim3(1), dim3(1), 0, s, (int*)nullptr, all_ok, 1);
        return ctxop::fail(c, "k_kzg_init", hipGetLastError());
    }
    const g16::FoldPlan fp = g16::fold_plan(n, 1);
    const kzg::Layout L = kzg::make_layout(n, flags, fp.part_bytes, fp.sum_bytes);
    // the workspaces first (an allocation synchronises the device); the borrowed stages keep their own grow-only buffers, which is why a
    // call is run once before it is captured
    void* ws = nullptr;
    if ((rc = ctxop::grow_kzg(c, L.total, &ws))) return rc;
    const bool shared = !msm::msm_args_bad(2 * n + 1, 2);
    if ((rc = ctxop::grow_msm(c, shared ? msm_workspace_bytes(1, 2 * n + 1, 2, 1) : msm_workspace_bytes(1, 2 * n + 1, 1, 0)))) return rc;   // the n-term call needs no more
    char* w = (char*)ws;
    int* flag = (int*)(w + L.flag);
    uint8_t *st = (uint8_t*)(w + L.st), *minf = (uint8_t*)(w + L.minf), *minf1 = (uint8_t*)(w + L.minf1);
    uint64_t *ms = (uint64_t*)(w + L.ms), *mp = (uint64_t*)(w + L.mp), *u = (uint64_t*)(w + L.u);
    uint64_t* row1 = shared ? ms + 4 * (2 * n + 1) : nullptr;
    uint64_t *mg1 = (uint64_t*)(w + L.mg1), *mg2 = (uint64_t*)(w + L.mg2), *ml = (uint64_t*)(w + L.ml);

    hipLaunchKernelGGL(k_kzg_init, dim3(1), dim3(1), 0, s, flag, all_ok, 0);
    if ((rc = ctxop::fail(c, "k_kzg_init", hipGetLastError()))) return rc;
    hipLaunchKernelGGL(k_kzg_g2, dim3(1), dim3(64), 0, s, (const uint64_t*)vk->g2, (const uint64_t*)vk->tau_g2, mg2);
    if ((rc = ctxop::fail(c, "k_kzg_g2", hipGetLastError()))) return rc;
    // 1. the points check: the statuses side by side, then one fold (-Q is valid exactly when Q is)
    if (L.n_status) {
        uint8_t* at = st;
        auto valid = [&](int which, const void* pts, const void* inf, size_t cnt) -> int {
            const int r = ctxop::valid(c, which, pts, inf, cnt, at, s);
            at += cnt;
            return r;
        };
        if (!(flags & ZKP_KZG_POINTS_CHECKED) && ((rc = valid(1, b->c, b->inf_c, n)) || (rc = valid(1, b->proof, b->inf_proof, n)))) return rc;
        if (!(flags & ZKP_KZG_VK_CHECKED) && ((rc = valid(1, vk->g1, nullptr, 1)) || (rc = valid(2, mg2, nullptr, 2)))) return rc;
        hipLaunchKernelGGL(k_kzg_status, dim3(blocks(L.n_status)), dim3(256), 0, s, st, L.n_status, flag);
        if ((rc = ctxop::fail(c, "k_kzg_status", hipGetLastError()))) return rc;
    }
    // 2. r_i and t_i (also what flags a zero (a, b) and a z >= r)
    hipLaunchKernelGGL(k_kzg_scalars, dim3(blocks(n)), dim3(256), 0, s, rand, (const uint64_t*)b->z, n, ms, row1, flag);
    if ((rc = ctxop::fail(c, "k_kzg_scalars", hipGetLastError()))) return rc;
    // 3. u = sum r_i y_i (also what flags a y >= r)
    if ((rc = ctxop::fail(c, "fr_fold", fr_fold(w + L.part, w + L.sum, ms, (const uint64_t*)b->y, n, 1, u, nullptr, flag, s)))) return rc;
    // 4. the larger MSM's points and its last scalar
    hipLaunchKernelGGL(k_kzg_place, dim3(blocks(24 * n + 12)), dim3(256), 0, s, (const uint64_t*)b->c, (const uint8_t*)b->inf_c, (const uint64_t*)b->proof,
                       (const uint8_t*)b->inf_proof, (const uint64_t*)vk->g1, (const uint64_t*)u, n, mp, minf, ms, row1);
    if ((rc = ctxop::fail(c, "k_kzg_place", hipGetLastError()))) return rc;
    // 5. sum r_i C_i + sum t_i pi_i - [u]g1, and sum r_i pi_i
    if (shared) {
        if ((rc = ctxop::msm_shared(c, 1, mp, minf, ms, 2 * n + 1, 2, mg1, minf1, s))) return rc;
    } else if ((rc = ctxop::msm(c, 1, mp, minf, ms, 2 * n + 1, 1, mg1, minf1, s)) ||
               (rc = ctxop::msm(c, 1, b->proof, b->inf_proof, ms, n, 1, mg1 + 12, minf1 + 1, s))) {
        return rc;
    }
    // 6. + 7. the two pairs, one final exponentiation, then the AND
    if ((rc = ctxop::miller_product(c, mg1, mg2, minf1, nullptr, 2, ml, s)) || (rc = ctxop::gt_is_one(c, ml, 1, ml + 72, flag + 1, s))) return rc;
    hipLaunchKernelGGL(k_kzg_finish, dim3(1), dim3(1), 0, s, flag, all_ok);
    return ctxop::fail(c, "k_kzg_finish", hipGetLastError());
}

}  // namespace zkp
