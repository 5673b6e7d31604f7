// zkp_poly.hip -- the batched Fr NTT (zkp_fr_ntt_batch) and the producer side of KZG (zkp_kzg_open_batch).
//
// NTT: one kernel, k_ntt_pass, launched once per pass of the plan (zkp_poly_plan.hpp: which bits a pass owns, what a tile is, why the
// passes work in place).  A workgroup of 256 threads takes a tile of 2^10 elements of 32 bytes into LDS (32 KiB, word-major and folded,
// lds_slot: the 32 lanes of a group touch 32 banks in every phase), then runs the pass's stages in ROUNDS: a thread takes four
// elements that differ in two tile bits into registers - four NAMED arrays, nothing indexed by a loop variable - runs the two
// radix-2 stages on them and puts them back.  Data stays canonical and the twiddles, read from the context's domain table w^i (the
// inverse reads w^(N - i); a smaller transform reads with a stride), stay in Montgomery form, so mont_mul(x, w) IS the canonical
// product.  The stage on bit 0 has twiddle one throughout and multiplies nothing.  The coset powers 7^i (forward, while
// loading the first pass) and 7^-i (inverse, while storing the last) are two products with entries of two 2^10-entry tables; the
// inverse's 2^-k is one more while storing.  Loads and stores are 8-byte accesses (the ABI promises uint64_t alignment) of runs of
// at least four records.  No atomics; the arithmetic is exact, so the result does not depend on the grid.
//
// Opening: y_j = f_j(z_j) and the inverted denominators 1 / (z_j - w^i) by fr_eval (zkp_kzg.hip) - they stay in the workspace -, then
// k_open_quot turns them IN PLACE into the quotient's evaluations q_i = (f_i - y) / (w^i - z), then one shared-bases MSM of the n
// rows over the N setup points.  Where z_j = w^m the inversion left a zero at slot m; there q_m = -z^-1 sum_{i != m} q_i w^i with
// z^-1 = w^(N - m) from the domain table.
//
// tests/poly_kernel_host.cpp compiles the KERNELS of this file for the host (ZKP_POLY_KERNELS_ONLY: one std::thread per lane, a barrier
// for __syncthreads) and runs them under ASan and UBSan against the Python model; the launch code below the kernels is left out there.
#ifndef ZKP_POLY_KERNELS_ONLY
#include "zkp_poly.hpp"

#include "zkp_kzg_plan.hpp"
#include "zkp_msm.hpp"
#include "zkp_msm_plan.hpp"
#endif
#include "zkp_fr.hpp"
#include "zkp_poly_plan.hpp"

namespace zkp {
namespace {

using fr::NW;
constexpr int TPB = (int)poly::TPB;
constexpr uint32_t TILE = 1u << poly::TILE_LOG2;
static_assert(TILE == 4 * poly::TPB, "a thread holds four elements of the tile");
constexpr fr::Roots ROOTS = fr::make_roots();

struct FrWords { uint32_t w[NW]; };
inline FrWords words_of(const uint32_t* v) {
    FrWords f;
    for (int i = 0; i < NW; i++) f.w[i] = v[i];
    return f;
}

__device__ __forceinline__ void tile_put(uint32_t* sh, uint32_t e, const uint32_t* v) {
    const uint32_t s = poly::lds_slot(e);
#pragma unroll
    for (int k = 0; k < NW; k++) sh[k * TILE + s] = v[k];
}
__device__ __forceinline__ void tile_get(uint32_t* v, const uint32_t* sh, uint32_t e) {
    const uint32_t s = poly::lds_slot(e);
#pragma unroll
    for (int k = 0; k < NW; k++) v[k] = sh[k * TILE + s];
}
__device__ __forceinline__ void table_get(uint32_t* v, const uint32_t* __restrict__ table, size_t at) {
#pragma unroll
    for (int k = 0; k < NW; k++) v[k] = table[at * NW + k];
}
// x <- x 7^i (inv = 0) or x 7^-i (inv = 1), i < 2^20
__device__ __forceinline__ void coset_mul(uint32_t* x, const uint32_t* __restrict__ coset, uint32_t i, uint32_t inv) {
    const uint32_t lo = i & ((1u << poly::COSET_LOG2) - 1), hi = i >> poly::COSET_LOG2;
    uint32_t w[NW];
    table_get(w, coset, ((size_t)(2 * inv) << poly::COSET_LOG2) + lo);
    fr::mont_mul(x, x, w);
    if (hi) {
        table_get(w, coset, ((size_t)(2 * inv + 1) << poly::COSET_LOG2) + hi);
        fr::mont_mul(x, x, w);
    }
}
// one radix-2 butterfly on the pair (a, b), twiddle table entry ti (0: one, no product)
template <bool DIT>
__device__ __forceinline__ void butterfly(uint32_t* a, uint32_t* b, const uint32_t* __restrict__ table, uint32_t tshift, uint32_t ti, bool has_twiddle) {
    uint32_t w[NW], d[NW];
    if (has_twiddle) table_get(w, table, (size_t)ti << tshift);
    if (DIT) {
        if (has_twiddle) fr::mont_mul(b, b, w);
        fr::sub(d, a, b);
        fr::add(a, a, b);
#pragma unroll
        for (int k = 0; k < NW; k++) b[k] = d[k];
    } else {
        fr::sub(d, a, b);
        fr::add(a, a, b);
        if (has_twiddle) fr::mont_mul(b, d, w);
        else {
#pragma unroll
            for (int k = 0; k < NW; k++) b[k] = d[k];
        }
    }
}

template <bool DIT>
__global__ __launch_bounds__(TPB) void k_ntt_pass(const uint64_t* in, uint64_t* out, const uint32_t* __restrict__ table, uint32_t tshift,
                                                  const uint32_t* __restrict__ coset, poly::Pass a, FrWords ninv) {
    __shared__ uint32_t sh[NW * TILE];
    const uint32_t q = threadIdx.x, wg = blockIdx.x;
    const uint32_t nmask = poly::low_mask(a.k);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t u = j * TPB + q;
        const uint64_t g = poly::element_index(a, wg, u);
        uint32_t v[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) v[k] = 0;
        if (g < a.total) {
            fr::wire_load(v, in + 4 * g);
            if (a.coset_in) coset_mul(v, coset, (uint32_t)g & nmask, 0);
        }
        tile_put(sh, u, v);
    }
    __syncthreads();
    const uint32_t rounds = poly::n_rounds(a);
#pragma unroll 1
    for (uint32_t r = 0; r < rounds; r++) {
        const poly::Round R = poly::round_of(a, r);
        const uint32_t e0 = poly::round_element(R, q, 0), e1 = poly::round_element(R, q, 1), e2 = poly::round_element(R, q, 2),
                       e3 = poly::round_element(R, q, 3);
        uint32_t x0[NW], x1[NW], x2[NW], x3[NW];
        tile_get(x0, sh, e0);
        tile_get(x1, sh, e1);
        tile_get(x2, sh, e2);
        tile_get(x3, sh, e3);
        // the stage on global bit 0 has twiddle one for every butterfly (uniform over the launch)
        const bool tw_lo = a.lo + R.pos != a.cl, tw_hi = true;
        if (DIT) {
            if (R.lo) {
                const uint32_t ti = poly::twiddle_index(a, wg, e0, R.pos);
                butterfly<true>(x0, x1, table, tshift, ti, tw_lo);
                butterfly<true>(x2, x3, table, tshift, ti, tw_lo);
            }
            if (R.hi) {
                butterfly<true>(x0, x2, table, tshift, poly::twiddle_index(a, wg, e0, R.pos + 1), tw_hi);
                butterfly<true>(x1, x3, table, tshift, poly::twiddle_index(a, wg, e1, R.pos + 1), tw_hi);
            }
        } else {
            if (R.hi) {
                butterfly<false>(x0, x2, table, tshift, poly::twiddle_index(a, wg, e0, R.pos + 1), tw_hi);
                butterfly<false>(x1, x3, table, tshift, poly::twiddle_index(a, wg, e1, R.pos + 1), tw_hi);
            }
            if (R.lo) {
                const uint32_t ti = poly::twiddle_index(a, wg, e0, R.pos);
                butterfly<false>(x0, x1, table, tshift, ti, tw_lo);
                butterfly<false>(x2, x3, table, tshift, ti, tw_lo);
            }
        }
        tile_put(sh, e0, x0);
        tile_put(sh, e1, x1);
        tile_put(sh, e2, x2);
        tile_put(sh, e3, x3);
        __syncthreads();
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t u = j * TPB + q;
        uint32_t e;
        uint64_t g;
        poly::store_map(a, wg, u, &e, &g);
        if (g >= a.total) continue;
        uint32_t v[NW];
        tile_get(v, sh, e);
        if (a.scale) fr::mont_mul(v, v, ninv.w);
        if (a.coset_out) coset_mul(v, coset, (uint32_t)g & nmask, 1);
        fr::wire_store(out + 4 * g, v);
    }
}

// coset[which][j], j < 2^10: 7^j, 7^(2^10 j), 7^-j, 7^-(2^10 j), Montgomery form, by the bits of j
__global__ void k_poly_coset(uint32_t* coset, FrWords g0, FrWords g1, FrWords g2, FrWords g3) {
    constexpr fr::Consts K = fr::make_consts();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, which = i >> poly::COSET_LOG2;
    if (which >= 4) return;
    uint32_t res[NW], b[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) {
        res[k] = K.one[k];
        b[k] = which == 0 ? g0.w[k] : which == 1 ? g1.w[k] : which == 2 ? g2.w[k] : g3.w[k];
    }
#pragma unroll 1
    for (uint32_t e = i & ((1u << poly::COSET_LOG2) - 1); e; e >>= 1) {
        if (e & 1) fr::mont_mul(res, res, b);
        fr::mont_mul(b, b, b);
    }
#pragma unroll
    for (int k = 0; k < NW; k++) coset[(size_t)i * NW + k] = res[k];
}

// the domain index of evaluation slot i, as zkp_kzg.hip's evaluation
__device__ __forceinline__ uint32_t domain_index(uint32_t i, uint32_t k, int bitrev) { return bitrev ? poly::bitrev(i, k) : i; }
// q[j N + i] <- (y_j - f_{j,i}) q[j N + i] where q holds 1 / (z_j - w^idx(i)) on entry; a zero there (z_j = w^idx(m), at most one m) gets
// -w^(N - idx(m)) sum_i q_i w^idx(i).  2^tp_log2 = min(N, 256) lanes share a polynomial, 256 >> tp_log2 polynomials a workgroup.
__global__ __launch_bounds__(TPB) void k_open_quot(const uint64_t* __restrict__ evals, const uint64_t* __restrict__ y, uint64_t* q,
                                                   const uint32_t* __restrict__ table, uint32_t tshift, uint32_t k, int bitrev, uint32_t n_poly,
                                                   uint32_t tp_log2) {
    __shared__ uint32_t sh[NW * TPB];
    __shared__ uint32_t hit[TPB];
    const uint32_t t = threadIdx.x, tp = 1u << tp_log2, li = t & (tp - 1), pg = t >> tp_log2, n_ev = 1u << k;
    const uint32_t j = blockIdx.x * (TPB >> tp_log2) + pg;
    if (li == 0) hit[pg] = 0;
    __syncthreads();
    uint32_t acc[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) acc[w] = 0;
    if (j < n_poly) {
        uint32_t yy[NW];
        fr::wire_load(yy, y + 4 * (size_t)j);
        for (uint32_t i = li; i < n_ev; i += tp) {
            const size_t e = ((size_t)j << k) + i;
            uint32_t di[NW], f[NW], w[NW], nz = 0;
            fr::wire_load(di, q + 4 * e);
#pragma unroll
            for (int c = 0; c < NW; c++) nz |= di[c];
            if (!nz) {
                hit[pg] = i + 1;   // one writer per polynomial: the w^i are distinct
                continue;
            }
            fr::wire_load(f, evals + 4 * e);
            fr::sub(f, yy, f);
            fr::mul(f, f, di);         // (y - f_i) / (z - w^i), canonical
            fr::wire_store(q + 4 * e, f);
            table_get(w, table, (size_t)domain_index(i, k, bitrev) << tshift);
            fr::mont_mul(f, f, w);     // q_i w^i, canonical
            fr::add(acc, acc, f);
        }
    }
#pragma unroll
    for (int c = 0; c < NW; c++) sh[c * TPB + t] = acc[c];
    __syncthreads();
    for (uint32_t s = tp >> 1; s >= 1; s >>= 1) {
        if (li < s) {
            uint32_t o[NW];
#pragma unroll
            for (int c = 0; c < NW; c++) o[c] = sh[c * TPB + t + s];
            fr::add(acc, acc, o);
#pragma unroll
            for (int c = 0; c < NW; c++) sh[c * TPB + t] = acc[c];
        }
        __syncthreads();
    }
    if (li != 0 || j >= n_poly || !hit[pg]) return;
    const uint32_t m = hit[pg] - 1, d = domain_index(m, k, bitrev);
    uint32_t w[NW];
    table_get(w, table, (size_t)((n_ev - d) & (n_ev - 1)) << tshift);
    fr::mont_mul(acc, acc, w);
    fr::neg(acc, acc);
    fr::wire_store(q + 4 * (((size_t)j << k) + m), acc);
}

}  // namespace

#ifndef ZKP_POLY_KERNELS_ONLY
hipError_t poly_coset_build(uint32_t* coset, hipStream_t s) {
    const uint32_t seven[NW] = {7, 0, 0, 0, 0, 0, 0, 0};
    FrWords g[4];
    fr::to_mont(g[0].w, seven);
    fr::mont_inv(g[2].w, g[0].w);
    for (int which = 0; which < 4; which += 2) {
        g[which + 1] = g[which];
        for (unsigned i = 0; i < poly::COSET_LOG2; i++) fr::mont_mul(g[which + 1].w, g[which + 1].w, g[which + 1].w);
    }
    hipLaunchKernelGGL(k_poly_coset, dim3((4u << poly::COSET_LOG2) / 256), dim3(256), 0, s, coset, g[0], g[1], g[2], g[3]);
    return hipGetLastError();
}

hipError_t fr_ntt(void* ws, const uint32_t* table, unsigned table_log2, const uint32_t* coset, const uint64_t* in, size_t n_poly, unsigned log2_n, int flags,
                  uint64_t* out, hipStream_t s) {
    const poly::Plan P = poly::make_plan(n_poly, log2_n, flags);
    if (!P.ok || (P.workspace && !ws)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)poly::ntt_tiles(n_poly, log2_n);
    const uint32_t tshift = table_log2 - log2_n;
    const FrWords ninv = words_of(ROOTS.inv_pow2[log2_n]);
    for (int p = 0; p < P.n_pass; p++) {
        const bool last = p == P.n_pass - 1;
        uint64_t* mid = P.workspace ? (uint64_t*)ws : out;
        const uint64_t* src = p == 0 ? in : mid;
        uint64_t* dst = last ? out : mid;
        if (P.pass[p].dit) hipLaunchKernelGGL(k_ntt_pass<true>, dim3(grid), dim3(TPB), 0, s, src, dst, table, tshift, coset, P.pass[p], ninv);
        else hipLaunchKernelGGL(k_ntt_pass<false>, dim3(grid), dim3(TPB), 0, s, src, dst, table, tshift, coset, P.pass[p], ninv);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

int kzg_open_dev(zkp_ctx* c, const void* lagrange, const uint64_t* evals, const uint64_t* z, size_t n, unsigned log2_n, int flags, uint64_t* out_y,
                 uint64_t* out_proof, uint8_t* out_inf, hipStream_t s) {
    if (!n) return 0;
    const size_t N = (size_t)1 << log2_n, slice = poly::open_slice(n, log2_n);
    const kzg::EvalLayout L = kzg::eval_layout(slice, log2_n);
    // the workspaces first (an allocation synchronises the device), then only launches
    void* ws = nullptr;
    const uint32_t* table = nullptr;
    unsigned table_log2 = 0;
    int rc;
    if ((rc = ctxop::grow_kzg(c, L.total, &ws)) || (rc = ctxop::grow_msm(c, msm_workspace_bytes(1, N, slice, 1))) ||
        (rc = ctxop::kzg_domain(c, log2_n, &table, &table_log2, s)))
        return rc;
    const int bitrev = (flags & ZKP_FR_EVAL_BITREV) ? 1 : 0;
    for (size_t at = 0; at < n; at += slice) {
        const size_t cnt = n - at < slice ? n - at : slice;
        const kzg::EvalLayout Ls = kzg::eval_layout(cnt, log2_n);   // fr_eval lays its regions out for cnt polynomials: a short last slice's differ
        const uint64_t* ev = evals + 4 * (at << log2_n);
        uint64_t* y = out_y + 4 * at;
        uint64_t* qs = (uint64_t*)((char*)ws + Ls.den);              // the inverted denominators, then the quotient
        if ((rc = ctxop::fail(c, "fr_eval", fr_eval(ws, table, table_log2, ev, z + 4 * at, cnt, log2_n, flags, y, s)))) return rc;
        hipLaunchKernelGGL(k_open_quot, dim3((unsigned)Ls.sum_blocks), dim3(TPB), 0, s, ev, (const uint64_t*)y, qs, table, table_log2 - log2_n, (uint32_t)log2_n,
                           bitrev, (uint32_t)cnt, (uint32_t)Ls.tp_log2);
        if ((rc = ctxop::fail(c, "k_open_quot", hipGetLastError()))) return rc;
        if ((rc = ctxop::msm_shared(c, 1, lagrange, nullptr, qs, N, cnt, out_proof + 12 * at, out_inf + at, s))) return rc;
    }
    return 0;
}

#endif

}  // namespace zkp
