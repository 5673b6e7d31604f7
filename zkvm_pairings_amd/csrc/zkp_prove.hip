// zkp_prove.hip -- the Fr sparse matrix times dense vectors product (zkp_fr_spmv_batch), the QAP quotient (zkp_groth16_quotient_batch)
// and the batched Groth16 prover (zkp_groth16_prove_batch); include/zkp_prove.h states what they compute.
//
// k_spmv: 2^t lanes share a row (zkp_prove_plan.hpp: t from nnz / n_rows on the host, adjacent lane groups on adjacent rows), a lane
// strides the row's entries: one 4-byte column index, one 32-byte value (consecutive lanes read consecutive values) and one 32-byte
// gather from the vector per entry.  Values and vector entries are canonical, so mont_mul(val, x) is val x / R; the lane sums are
// added through LDS (word-major: the 32 lanes of a group touch 32 banks), and one product with R^2 per output leaves the canonical
// sum.  The vector index is the grid's y dimension (strided when n exceeds it): the lanes of a workgroup then gather from ONE vector,
// whose hot columns stay in L2.  The kernel never reads outside the matrix arrays or the vector: a row bound beyond nnz is clamped
// and a column >= n_cols skipped, and either ORs 1 into *bad - a malformed matrix from a _dev caller cannot fault the device.
// No atomics on field data (the one atomicOr is that flag); exact, so the bytes do not depend on t or the grid.
//
// k_prove_sat compares a_k b_k with c_k on the evaluations and clears sat[j] (every writer stores the same byte); k_prove_quot is the
// pointwise a_i <- (a_i b_i - c_i) / (7^N - 1) on the coset, in bit-reversed order like every transform here, so that none of the
// seven NTTs (fr_ntt, zkp_poly.hip) needs a workspace.  The small k_prove_* kernels below serve the assembly: r, s and -r s of a
// proof, the padded copies of l_query and h_query, one point repeated n times, and the infinity of a scalar multiple of an infinite
// point.
//
// tests/prove_kernel_host.cpp compiles the KERNELS of this file for the host (ZKP_PROVE_KERNELS_ONLY: one std::thread per lane, a
// barrier for __syncthreads) and runs them under ASan and UBSan against the Python model; the launch code below is left out there.
#ifndef ZKP_PROVE_KERNELS_ONLY
#include "zkp_prove.hpp"

#include "zkp_msm.hpp"
#endif
#include "zkp_fr.hpp"
#include "zkp_prove_plan.hpp"

namespace zkp {
namespace {

using fr::NW;
constexpr int PTPB = (int)prove::TPB;

struct FrK { uint32_t w[NW]; };

__global__ __launch_bounds__(PTPB) void k_spmv(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, const uint64_t* __restrict__ val,
                                               const uint64_t* __restrict__ x, uint64_t* out, uint32_t n_rows, uint32_t n_cols, uint32_t nnz, uint32_t n,
                                               uint32_t out_stride, uint32_t t, uint32_t brv_log2, int* bad) {
    __shared__ uint32_t sh[NW * PTPB];
    const uint32_t q = threadIdx.x, tp = 1u << t, li = prove::spmv_lane(q, t), k = prove::spmv_row(blockIdx.x, q, t);
    uint32_t lo = 0, hi = 0, flag = 0;
    if (k < n_rows) {
        lo = row_ptr[k];
        hi = row_ptr[k + 1];
        if (hi > nnz) { hi = nnz; flag = 1; }
        if (lo > hi) { lo = hi; flag = 1; }
    }
#pragma unroll 1
    for (uint32_t j = blockIdx.y; j < n; j += gridDim.y) {
        const uint64_t* xj = x + 4 * (size_t)j * n_cols;
        uint32_t acc[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) acc[w] = 0;
#pragma unroll 1
        for (uint32_t e = lo + li; e < hi; e += tp) {   // hi <= nnz < 2^31: e + tp cannot wrap
            const uint32_t ci = col[e];
            if (ci >= n_cols) { flag = 1; continue; }
            uint32_t v[NW], xx[NW];
            fr::wire_load(v, val + 4 * (size_t)e);
            fr::wire_load(xx, xj + 4 * (size_t)ci);
            fr::mont_mul(v, v, xx);
            fr::add(acc, acc, v);
        }
#pragma unroll
        for (int w = 0; w < NW; w++) sh[w * PTPB + q] = acc[w];
        __syncthreads();
        for (uint32_t s = tp >> 1; s >= 1; s >>= 1) {
            if (li < s) {
                uint32_t o[NW];
#pragma unroll
                for (int w = 0; w < NW; w++) o[w] = sh[w * PTPB + q + s];
                fr::add(acc, acc, o);
#pragma unroll
                for (int w = 0; w < NW; w++) sh[w * PTPB + q] = acc[w];
            }
            __syncthreads();
        }
        if (li == 0 && k < out_stride) {
            fr::to_mont(acc, acc);   // (sum / R) R^2 / R: rows from n_rows on hold zero
            const uint32_t slot = brv_log2 ? poly::bitrev(k, brv_log2) : k;
            fr::wire_store(out + 4 * ((size_t)j * out_stride + slot), acc);
        }
    }
    if (flag) atomicOr(bad, 1);
}

__global__ void k_prove_sat_init(uint8_t* sat, uint32_t n) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) sat[j] = 1;
}
// sat[i >> k] <- 0 where a_i b_i != c_i (any order of the evaluations: all three share it)
__global__ __launch_bounds__(PTPB) void k_prove_sat(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const uint64_t* __restrict__ c,
                                                    uint32_t total, uint32_t k, uint8_t* sat) {
    const uint32_t i = blockIdx.x * PTPB + threadIdx.x;
    if (i >= total) return;
    uint32_t x[NW], y[NW];
    fr::wire_load(x, a + 4 * (size_t)i);
    fr::wire_load(y, b + 4 * (size_t)i);
    fr::mont_mul(x, x, y);           // a b / R
    fr::wire_load(y, c + 4 * (size_t)i);
    fr::from_mont(y, y);             // c / R
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) d |= x[w] ^ y[w];
    if (d) sat[i >> k] = 0;
}
// a_i <- (a_i b_i - c_i) kinv, kinv = (7^N - 1)^-1 in Montgomery form
__global__ __launch_bounds__(PTPB) void k_prove_quot(uint64_t* a, const uint64_t* __restrict__ b, const uint64_t* __restrict__ c, uint32_t total, FrK kinv) {
    const uint32_t i = blockIdx.x * PTPB + threadIdx.x;
    if (i >= total) return;
    uint32_t x[NW], y[NW];
    fr::wire_load(x, a + 4 * (size_t)i);
    fr::wire_load(y, b + 4 * (size_t)i);
    fr::mul(x, x, y);
    fr::wire_load(y, c + 4 * (size_t)i);
    fr::sub(x, x, y);
    fr::mont_mul(x, x, kinv.w);
    fr::wire_store(a + 4 * (size_t)i, x);
}
// rs[j] = r_j | s_j -> r, s, -r s
__global__ void k_prove_rs(const uint64_t* __restrict__ rs, uint32_t n, uint64_t* r, uint64_t* s, uint64_t* nrs) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint32_t x[NW], y[NW];
    fr::wire_load(x, rs + 8 * (size_t)j);
    fr::wire_load(y, rs + 8 * (size_t)j + 4);
    fr::wire_store(r + 4 * (size_t)j, x);
    fr::wire_store(s + 4 * (size_t)j, y);
    fr::mul(x, x, y);
    fr::neg(x, x);
    fr::wire_store(nrs + 4 * (size_t)j, x);
}
// word w of the infinite G1 point as the library writes it: (0, 1)
__device__ __forceinline__ uint64_t g1_inf_word(uint32_t w) { return w == 6 ? 1u : 0u; }
// dst[i] (total G1 points and flags): `lead` infinite entries, then the n_src points of src (src_inf may be null), then infinite ones
__global__ void k_prove_pad(const uint64_t* __restrict__ src, const uint8_t* __restrict__ src_inf, uint32_t n_src, uint32_t lead, uint32_t total,
                            uint64_t* dst, uint8_t* dst_inf) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const bool real = i >= lead && i - lead < n_src;
    const uint8_t inf = real ? (src_inf ? (src_inf[i - lead] ? 1 : 0) : 0) : 1;
    for (uint32_t w = 0; w < 12; w++) dst[12 * (size_t)i + w] = inf ? g1_inf_word(w) : src[12 * (size_t)(i - lead) + w];
    dst_inf[i] = inf;
}
// out[j] = pt (words u64 each) for j < n
__global__ void k_prove_bcast(const uint64_t* __restrict__ pt, uint32_t words, uint32_t n, uint64_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * words) return;
    out[i] = pt[i % words];
}
// a scalar multiple of an infinite point is infinite: where base_inf[j] is set, out[j] <- (0, 1) and out_inf[j] <- 1
__global__ void k_prove_mulinf(const uint8_t* __restrict__ base_inf, uint32_t n, uint64_t* out, uint8_t* out_inf) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !base_inf[j]) return;
    for (uint32_t w = 0; w < 12; w++) out[12 * (size_t)j + w] = g1_inf_word(w);
    out_inf[j] = 1;
}

}  // namespace

#ifndef ZKP_PROVE_KERNELS_ONLY
namespace {
inline unsigned blocks(size_t n, unsigned tpb = 256) { return (unsigned)((n + tpb - 1) / tpb); }

// (7^N - 1)^-1 in Montgomery form
FrK coset_vanishing_inverse(unsigned log2_n) {
    constexpr fr::Consts K = fr::make_consts();
    const uint32_t seven[NW] = {7, 0, 0, 0, 0, 0, 0, 0};
    FrK g;
    fr::to_mont(g.w, seven);
    for (unsigned i = 0; i < log2_n; i++) fr::mont_mul(g.w, g.w, g.w);
    fr::sub(g.w, g.w, K.one);
    fr::mont_inv(g.w, g.w);
    return g;
}

struct Tables {
    const uint32_t *table = nullptr, *coset = nullptr;
    unsigned table_log2 = 0;
};

// one slice of the quotient: h of cnt witnesses into a (cnt x N), b and cc are scratch of the same size; asynchronous on s
int quotient_slice(zkp_ctx* c, const zkp_r1cs* r, const Tables& T, const FrK& kinv, const uint64_t* wit, size_t cnt, uint64_t* a, uint64_t* b, uint64_t* cc,
                   uint8_t* sat, hipStream_t s) {
    const unsigned k = r->log2_n;
    const size_t N = (size_t)1 << k, total = cnt * N;
    int* bad = ctxop::validation_word(c);
    int rc;
    hipLaunchKernelGGL(k_prove_sat_init, dim3(blocks(cnt)), dim3(256), 0, s, sat, (uint32_t)cnt);
    if ((rc = ctxop::fail(c, "k_prove_sat_init", hipGetLastError()))) return rc;
    if ((rc = ctxop::fail(c, "fr_spmv", fr_spmv(&r->a, wit, cnt, N, k, a, bad, s))) || (rc = ctxop::fail(c, "fr_spmv", fr_spmv(&r->b, wit, cnt, N, k, b, bad, s))) ||
        (rc = ctxop::fail(c, "fr_spmv", fr_spmv(&r->c, wit, cnt, N, k, cc, bad, s))))
        return rc;
    hipLaunchKernelGGL(k_prove_sat, dim3(blocks(total, PTPB)), dim3(PTPB), 0, s, (const uint64_t*)a, (const uint64_t*)b, (const uint64_t*)cc, (uint32_t)total,
                       (uint32_t)k, sat);
    if ((rc = ctxop::fail(c, "k_prove_sat", hipGetLastError()))) return rc;
    uint64_t* const ev[3] = {a, b, cc};
    for (int pass = 0; pass < 2; pass++)   // evaluations -> coefficients -> evaluations on the coset, bit-reversed on the evaluation side
        for (int i = 0; i < 3; i++)
            if ((rc = ctxop::fail(c, "fr_ntt", fr_ntt(nullptr, T.table, T.table_log2, T.coset, ev[i], cnt, k,
                                                      pass == 0 ? poly::NTT_INVERSE | poly::NTT_BITREV : poly::NTT_COSET | poly::NTT_BITREV, ev[i], s))))
                return rc;
    hipLaunchKernelGGL(k_prove_quot, dim3(blocks(total, PTPB)), dim3(PTPB), 0, s, a, (const uint64_t*)b, (const uint64_t*)cc, (uint32_t)total, kinv);
    if ((rc = ctxop::fail(c, "k_prove_quot", hipGetLastError()))) return rc;
    return ctxop::fail(c, "fr_ntt", fr_ntt(nullptr, T.table, T.table_log2, T.coset, a, cnt, k, poly::NTT_INVERSE | poly::NTT_COSET | poly::NTT_BITREV, a, s));
}

int tables(zkp_ctx* c, unsigned log2_n, Tables* T, hipStream_t s) {
    if (int rc = ctxop::kzg_domain(c, log2_n, &T->table, &T->table_log2, s)) return rc;
    return ctxop::poly_coset(c, &T->coset, s);
}
}  // namespace

hipError_t fr_spmv(const zkp_fr_csr* mat, const uint64_t* x, size_t n, size_t out_stride, unsigned brv_log2, uint64_t* out, int* bad, hipStream_t s) {
    const prove::SpmvGrid g = prove::spmv_grid(mat->nnz, mat->n_rows, n, out_stride);
    hipLaunchKernelGGL(k_spmv, dim3(g.x, g.y), dim3(PTPB), 0, s, (const uint32_t*)mat->row_ptr, (const uint32_t*)mat->col, (const uint64_t*)mat->val, x, out,
                       (uint32_t)mat->n_rows, (uint32_t)mat->n_cols, (uint32_t)mat->nnz, (uint32_t)n, (uint32_t)out_stride, g.t, brv_log2, bad);
    return hipGetLastError();
}

int groth16_quotient_dev(zkp_ctx* c, const zkp_r1cs* r, const uint64_t* witness, size_t n, uint64_t* out_h, uint8_t* out_sat, hipStream_t s) {
    if (!n) return 0;
    const size_t m = r->a.n_cols, N = (size_t)1 << r->log2_n, S = prove::slice(n, m, r->log2_n);
    const prove::Layout L = prove::layout(S, m, r->log2_n, false);
    // the workspaces first (an allocation synchronises the device), then only launches
    void* ws = nullptr;
    Tables T;
    int rc;
    if ((rc = ctxop::grow_prove(c, L.total, &ws)) || (rc = tables(c, r->log2_n, &T, s))) return rc;
    const FrK kinv = coset_vanishing_inverse(r->log2_n);
    for (size_t at = 0; at < n; at += S) {
        const size_t cnt = n - at < S ? n - at : S;
        if ((rc = quotient_slice(c, r, T, kinv, witness + 4 * at * m, cnt, out_h + 4 * at * N, (uint64_t*)((char*)ws + L.b_ev), (uint64_t*)((char*)ws + L.c_ev),
                                 out_sat + at, s)))
            return rc;
    }
    return 0;
}

int groth16_prove_dev(zkp_ctx* c, const zkp_r1cs* r, const zkp_groth16_pk* pk, const uint64_t* witness, const uint64_t* rs, size_t n, uint64_t* out_a,
                      uint8_t* out_inf_a, uint64_t* out_b, uint8_t* out_inf_b, uint64_t* out_c, uint8_t* out_inf_c, uint8_t* out_sat, hipStream_t s) {
    if (!n) return 0;
    const size_t m = r->a.n_cols, N = (size_t)1 << r->log2_n, l = r->n_inputs, S = prove::slice(n, m, r->log2_n);
    const prove::Layout L = prove::layout(S, m, r->log2_n, true);
    size_t msm_bytes = msm_workspace_bytes(1, m, S, 1);
    for (const size_t b : {msm_workspace_bytes(2, m, S, 1), msm_workspace_bytes(1, N, S, 1)}) msm_bytes = b > msm_bytes ? b : msm_bytes;
    // the workspaces first (an allocation synchronises the device), then only launches
    void* wsv = nullptr;
    Tables T;
    int rc;
    if ((rc = ctxop::grow_prove(c, L.total, &wsv)) || (rc = ctxop::grow_msm(c, msm_bytes)) || (rc = tables(c, r->log2_n, &T, s))) return rc;
    char* const ws = (char*)wsv;
    const FrK kinv = coset_vanishing_inverse(r->log2_n);
    uint64_t *const a_ev = (uint64_t*)(ws + L.a_ev), *const b_ev = (uint64_t*)(ws + L.b_ev), *const c_ev = (uint64_t*)(ws + L.c_ev);
    uint64_t *const l_pts = (uint64_t*)(ws + L.l_pts), *const h_pts = (uint64_t*)(ws + L.h_pts);
    uint8_t *const l_inf = (uint8_t*)(ws + L.l_inf), *const h_inf = (uint8_t*)(ws + L.h_inf);
    uint64_t *const sc_r = (uint64_t*)(ws + L.sc_r), *const sc_s = (uint64_t*)(ws + L.sc_s), *const sc_nrs = (uint64_t*)(ws + L.sc_nrs);
    uint64_t *g1[8], *g2[3];
    uint8_t *i1[8], *i2[3];
    for (int i = 0; i < 8; i++) { g1[i] = (uint64_t*)(ws + L.g1[i]); i1[i] = (uint8_t*)(ws + L.g1_inf[i]); }
    for (int i = 0; i < 3; i++) { g2[i] = (uint64_t*)(ws + L.g2[i]); i2[i] = (uint8_t*)(ws + L.g2_inf[i]); }
    // once per call: l_query behind n_inputs + 1 infinite entries (the witness rows then serve unchanged), h_query and one infinite entry
    hipLaunchKernelGGL(k_prove_pad, dim3(blocks(m)), dim3(256), 0, s, (const uint64_t*)pk->l_query, (const uint8_t*)pk->l_inf, (uint32_t)(m - l - 1), (uint32_t)(l + 1),
                       (uint32_t)m, l_pts, l_inf);
    hipLaunchKernelGGL(k_prove_pad, dim3(blocks(N)), dim3(256), 0, s, (const uint64_t*)pk->h_query, (const uint8_t*)nullptr, (uint32_t)(N - 1), 0u, (uint32_t)N, h_pts,
                       h_inf);
    if ((rc = ctxop::fail(c, "k_prove_pad", hipGetLastError()))) return rc;
    auto bcast = [&](const void* pt, uint32_t words, size_t cnt, uint64_t* out) {
        hipLaunchKernelGGL(k_prove_bcast, dim3(blocks(cnt * words)), dim3(256), 0, s, (const uint64_t*)pt, words, (uint32_t)cnt, out);
        return ctxop::fail(c, "k_prove_bcast", hipGetLastError());
    };
    auto mulinf = [&](const uint8_t* base_inf, size_t cnt, uint64_t* out, uint8_t* out_inf) {
        hipLaunchKernelGGL(k_prove_mulinf, dim3(blocks(cnt)), dim3(256), 0, s, base_inf, (uint32_t)cnt, out, out_inf);
        return ctxop::fail(c, "k_prove_mulinf", hipGetLastError());
    };
    for (size_t at = 0; at < n; at += S) {
        const size_t cnt = n - at < S ? n - at : S;
        const uint64_t* wit = witness + 4 * at * m;
        uint64_t *const A = out_a + 12 * at, *const B = out_b + 24 * at, *const C = out_c + 12 * at;
        uint8_t *const iA = out_inf_a + at, *const iB = out_inf_b + at, *const iC = out_inf_c + at;
        hipLaunchKernelGGL(k_prove_rs, dim3(blocks(cnt)), dim3(256), 0, s, rs + 8 * at, (uint32_t)cnt, sc_r, sc_s, sc_nrs);
        if ((rc = ctxop::fail(c, "k_prove_rs", hipGetLastError()))) return rc;
        if ((rc = quotient_slice(c, r, T, kinv, wit, cnt, a_ev, b_ev, c_ev, out_sat + at, s))) return rc;
        // A = alpha + sum_i z_i a_query_i + [r] delta
        if ((rc = ctxop::msm_shared(c, 1, pk->a_query, pk->a_inf, wit, m, cnt, g1[0], i1[0], s)) || (rc = ctxop::mul(c, 1, pk->delta_g1, 0, sc_r, cnt, g1[1], i1[1], s)) ||
            (rc = ctxop::add(c, 1, g1[0], i1[0], g1[1], i1[1], cnt, g1[2], i1[2], s)) || (rc = bcast(pk->alpha_g1, 12, cnt, g1[3])) ||
            (rc = ctxop::add(c, 1, g1[2], i1[2], g1[3], nullptr, cnt, A, iA, s)))
            return rc;
        // B = beta_g2 + sum_i z_i b_g2_query_i + [s] delta_g2
        if ((rc = ctxop::msm_shared(c, 2, pk->b_g2_query, pk->b_g2_inf, wit, m, cnt, g2[0], i2[0], s)) ||
            (rc = ctxop::mul(c, 2, pk->delta_g2, 0, sc_s, cnt, g2[1], i2[1], s)) || (rc = ctxop::add(c, 2, g2[0], i2[0], g2[1], i2[1], cnt, g2[2], i2[2], s)) ||
            (rc = bcast(pk->beta_g2, 24, cnt, g2[0])) || (rc = ctxop::add(c, 2, g2[2], i2[2], g2[0], nullptr, cnt, B, iB, s)))
            return rc;
        // B1 = beta_g1 + sum_i z_i b_g1_query_i + [s] delta_g1, into g1[4]
        if ((rc = ctxop::msm_shared(c, 1, pk->b_g1_query, pk->b_g1_inf, wit, m, cnt, g1[0], i1[0], s)) ||
            (rc = ctxop::mul(c, 1, pk->delta_g1, 0, sc_s, cnt, g1[1], i1[1], s)) || (rc = ctxop::add(c, 1, g1[0], i1[0], g1[1], i1[1], cnt, g1[2], i1[2], s)) ||
            (rc = bcast(pk->beta_g1, 12, cnt, g1[3])) || (rc = ctxop::add(c, 1, g1[2], i1[2], g1[3], nullptr, cnt, g1[4], i1[4], s)))
            return rc;
        // C = sum_{i > l} z_i l_query_i + sum_i h_i h_query_i + [s] A + [r] B1 - [r s] delta
        if ((rc = ctxop::msm_shared(c, 1, l_pts, l_inf, wit, m, cnt, g1[0], i1[0], s)) || (rc = ctxop::msm_shared(c, 1, h_pts, h_inf, a_ev, N, cnt, g1[1], i1[1], s)) ||
            (rc = ctxop::add(c, 1, g1[0], i1[0], g1[1], i1[1], cnt, g1[2], i1[2], s)) || (rc = ctxop::mul(c, 1, A, 12, sc_s, cnt, g1[3], i1[3], s)) ||
            (rc = mulinf(iA, cnt, g1[3], i1[3])) || (rc = ctxop::add(c, 1, g1[2], i1[2], g1[3], i1[3], cnt, g1[5], i1[5], s)) ||
            (rc = ctxop::mul(c, 1, g1[4], 12, sc_r, cnt, g1[6], i1[6], s)) || (rc = mulinf(i1[4], cnt, g1[6], i1[6])) ||
            (rc = ctxop::add(c, 1, g1[5], i1[5], g1[6], i1[6], cnt, g1[7], i1[7], s)) || (rc = ctxop::mul(c, 1, pk->delta_g1, 0, sc_nrs, cnt, g1[0], i1[0], s)) ||
            (rc = ctxop::add(c, 1, g1[7], i1[7], g1[0], i1[0], cnt, C, iC, s)))
            return rc;
    }
    return 0;
}
#endif

}  // namespace zkp
