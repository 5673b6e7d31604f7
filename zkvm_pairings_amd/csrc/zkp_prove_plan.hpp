// zkp_prove_plan.hpp -- the PURE index arithmetic of the Fr sparse matrix-vector product (zkp_fr_spmv_batch), of the QAP quotient and
// of the batched Groth16 prover (include/zkp_prove.h): the argument limits, how many lanes share a row, which lane group owns a row,
// the grids, the slices and the workspace regions.  No HIP type, no allocation, no I/O.  zkp_prove.hip compiles this text for the
// device; tests/prove_plan_check.cpp compiles it with g++ -fsanitize=address,undefined and walks it up to the ABI maxima.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zkp_poly_plan.hpp"   // poly::bitrev: the slot of a row in the quotient's bit-reversed evaluations

#if defined(__HIPCC__)
#define ZKP_PROVE_HD __host__ __device__ __forceinline__
#else
#define ZKP_PROVE_HD inline
#endif

namespace zkp {
namespace prove {

constexpr unsigned TPB = 256;
constexpr unsigned MAX_T = 6;                         // at most a wavefront shares a row
constexpr unsigned MIN_LOG2 = 1, MAX_LOG2 = 20;       // of the prover's domain
constexpr size_t MAX_COLS = (size_t)1 << 22;          // m
constexpr size_t MAX_NNZ = 0x7fffffffu;
constexpr size_t MAX_STRIDE = (size_t)1 << MAX_LOG2;  // out_stride of the product
constexpr size_t MAX_OUT = (size_t)1 << 26;           // n * out_stride of one product: the NTT's total
constexpr size_t MAX_N = 0x7fffffffu;
constexpr size_t SLICE_TERMS = (size_t)1 << 22;       // max(m, N) * proofs of one slice
constexpr unsigned MAX_GRID_Y = 65535;

constexpr bool csr_args_bad(size_t n_rows, size_t n_cols, size_t nnz) { return n_cols > MAX_COLS || nnz > MAX_NNZ || n_rows > MAX_STRIDE; }
constexpr bool spmv_args_bad(size_t n_rows, size_t n_cols, size_t nnz, size_t n, size_t out_stride) {
    return csr_args_bad(n_rows, n_cols, nnz) || out_stride < n_rows || out_stride > MAX_STRIDE || n > MAX_N || (out_stride && n > MAX_OUT / out_stride);
}
// the shape of an R1CS: (n_rows, n_cols, nnz) of the three matrices
constexpr bool r1cs_args_bad(unsigned log2_n, size_t n_inputs, size_t ra, size_t ca, size_t za, size_t rb, size_t cb, size_t zb, size_t rc, size_t cc,
                             size_t zc, size_t n) {
    return log2_n < MIN_LOG2 || log2_n > MAX_LOG2 || ra > ((size_t)1 << log2_n) || ra != rb || ra != rc || ca != cb || ca != cc || n_inputs >= ca ||
           ca > MAX_COLS || za > MAX_NNZ || zb > MAX_NNZ || zc > MAX_NNZ || n > MAX_N;
}

// 2^t lanes share a row: the smallest t with 2^t >= nnz / n_rows (rounded up), at most MAX_T.  Known from the arguments alone.
constexpr unsigned spmv_t(size_t nnz, size_t n_rows) {
    const size_t mean = n_rows ? (nnz + n_rows - 1) / n_rows : 0;
    unsigned t = 0;
    while (t < MAX_T && ((size_t)1 << t) < mean) t++;
    return t;
}
// adjacent lane groups take adjacent rows: row k belongs to group k % (TPB >> t) of workgroup k / (TPB >> t); the grid covers the
// out_stride output slots (the ones from n_rows on are zeroed), its y dimension strides the vectors
struct SpmvGrid {
    unsigned t = 0, x = 0, y = 0;
};
constexpr SpmvGrid spmv_grid(size_t nnz, size_t n_rows, size_t n, size_t out_stride) {
    SpmvGrid g;
    g.t = spmv_t(nnz, n_rows);
    const size_t per = TPB >> g.t;
    g.x = (unsigned)((out_stride + per - 1) / per);
    g.y = (unsigned)(n < MAX_GRID_Y ? n : MAX_GRID_Y);
    return g;
}
ZKP_PROVE_HD uint32_t spmv_row(uint32_t wg, uint32_t thread, uint32_t t) { return wg * (TPB >> t) + (thread >> t); }
ZKP_PROVE_HD uint32_t spmv_lane(uint32_t thread, uint32_t t) { return thread & ((1u << t) - 1u); }
// slices of whole proofs: max(m, N) * proofs <= SLICE_TERMS, at least one proof
constexpr size_t slice(size_t n, size_t m, unsigned log2_n) {
    const size_t big = m > ((size_t)1 << log2_n) ? m : ((size_t)1 << log2_n);
    const size_t per = SLICE_TERMS / big ? SLICE_TERMS / big : 1;
    return n < per ? n : per;
}

// the workspace of one slice of S proofs.  Offsets in bytes, every region rounded up to 256.
struct Layout {
    size_t a_ev = 0, b_ev = 0, c_ev = 0;       // S x N Fr each: the evaluations, then h in a_ev (the quotient call keeps a_ev in out_h)
    size_t l_pts = 0, l_inf = 0;               // m G1 + m bytes: l_query behind n_inputs + 1 infinite entries
    size_t h_pts = 0, h_inf = 0;               // N G1 + N bytes: h_query and one infinite entry
    size_t sc_r = 0, sc_s = 0, sc_nrs = 0;     // S Fr each: r, s, -r s
    size_t g1[8] = {}, g1_inf[8] = {};         // S G1 (+ S bytes) each: temporaries of the assembly
    size_t g2[3] = {}, g2_inf[3] = {};         // S G2 (+ S bytes) each
    size_t total = 0;
};
constexpr size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr Layout layout(size_t S, size_t m, unsigned log2_n, bool prover) {
    Layout L;
    const size_t N = (size_t)1 << log2_n;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o = at; at += up256(bytes); return o; };
    if (prover) L.a_ev = take(S * N * 32);
    L.b_ev = take(S * N * 32);
    L.c_ev = take(S * N * 32);
    if (prover) {
        L.l_pts = take(m * 96);
        L.l_inf = take(m);
        L.h_pts = take(N * 96);
        L.h_inf = take(N);
        L.sc_r = take(S * 32);
        L.sc_s = take(S * 32);
        L.sc_nrs = take(S * 32);
        for (int i = 0; i < 8; i++) { L.g1[i] = take(S * 96); L.g1_inf[i] = take(S); }
        for (int i = 0; i < 3; i++) { L.g2[i] = take(S * 192); L.g2_inf[i] = take(S); }
    }
    L.total = at;
    return L;
}

}  // namespace prove
}  // namespace zkp
