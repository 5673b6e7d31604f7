// zkp_kzg_plan.hpp -- the host side's PURE arithmetic of the batched Fr inversion (zkp_fr_invert_batch), of the barycentric evaluation
// (zkp_fr_eval_batch) and of the batch KZG opening verifier (zkp_kzg_verify_batch): the argument limits, the grids and the layouts of
// the workspace.  No HIP type, no allocation, no I/O: included by zkp_kzg.hip and zkp_pairings.hip (the product) and compiled with
// g++ -fsanitize=address,undefined by tests/test_kzg_cpu.py, which walks it over the sizes the C ABI admits.
//
// All three calls share ONE grow-only workspace of the context; a call lays its regions out from offset 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkp {
namespace kzg {

constexpr size_t INV_MAX = 0x7fffffff;           // n of zkp_fr_invert_batch
constexpr size_t INV_RUN = 4;                    // consecutive elements of a thread (zkp_fr.hpp: INV_RUN)
constexpr size_t INV_TPB = 256;                  // threads of a workgroup
constexpr size_t INV_BLOCK = INV_RUN * INV_TPB;  // elements of a workgroup: 1024
constexpr unsigned EVAL_MAX_LOG2 = 20;           // log2 of the evaluations of a polynomial
constexpr size_t EVAL_MAX_TOTAL = (size_t)1 << 26;   // n_poly * N
constexpr int EVAL_BITREV = 1, EVAL_ALL_FLAGS = 1;
constexpr size_t MAX_OPENINGS = (size_t)1 << 22; // n of the verifier: its MSM has 2 rows of 2 n + 1 terms, the MSM takes 2^24 (n = 2^22 itself: two calls)
constexpr int POINTS_CHECKED = 1, VK_CHECKED = 2, ALL_FLAGS = 3;
constexpr size_t ML_RECORDS = 2;                 // the Miller value of the two pairs, then Gt

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

constexpr bool inv_args_bad(size_t n) { return n > INV_MAX; }
// the inversion of n >= 1 elements: `blocks` workgroups of INV_BLOCK elements each leave one 32-byte total; the middle launch - one
// workgroup, each thread a run of `mid_run` consecutive totals - keeps their prefix products beside them
struct InvPlan {
    size_t blocks = 0, mid_run = 0, mid_threads = 0;
    size_t tot = 0, pre = 0, total = 0;          // byte offsets of the totals and of their prefix products; the size
};
inline InvPlan inv_plan(size_t n) {
    InvPlan p;
    p.blocks = (n + INV_BLOCK - 1) / INV_BLOCK;
    p.mid_run = (p.blocks + INV_TPB - 1) / INV_TPB;
    p.mid_threads = p.mid_run ? (p.blocks + p.mid_run - 1) / p.mid_run : 0;
    p.tot = 0;
    p.pre = align256(p.blocks * 32);
    p.total = p.pre + align256(p.blocks * 32);
    return p;
}

constexpr bool eval_args_bad(size_t n_poly, unsigned log2_n, int flags) {
    return log2_n > EVAL_MAX_LOG2 || (flags & ~EVAL_ALL_FLAGS) || n_poly > (EVAL_MAX_TOTAL >> log2_n);
}
inline size_t domain_bytes(unsigned log2_n) { return (size_t)32 << log2_n; }   // the table omega^i, Montgomery form (its own allocation)
// the evaluation of n_poly >= 1 polynomials: the inversion's regions, then one 32-byte denominator per evaluation
struct EvalLayout {
    InvPlan inv;
    size_t den = 0, total = 0;
    unsigned tp_log2 = 0;                        // lanes that share a polynomial in the sum: min(N, 256)
    size_t sum_blocks = 0;
};
inline EvalLayout eval_layout(size_t n_poly, unsigned log2_n) {
    EvalLayout L;
    const size_t evals = n_poly << log2_n;
    L.inv = inv_plan(evals);
    L.den = L.inv.total;
    L.total = L.den + align256(evals * 32);
    L.tp_log2 = log2_n < 8 ? log2_n : 8;
    const size_t per = INV_TPB >> L.tp_log2;
    L.sum_blocks = (n_poly + per - 1) / per;
    return L;
}

constexpr bool args_bad(size_t n, int flags) { return n > MAX_OPENINGS || (flags & ~ALL_FLAGS); }
struct Layout {
    size_t n_status = 0;   // status bytes of the points check: C and pi (2 n) unless POINTS_CHECKED; g1, -g2, [tau]g2 (3) unless VK_CHECKED
    // byte offsets, every region 256-byte aligned
    size_t flag = 0;       // int32 [0]: every point valid, every z and y < r, no zero (a, b); [1]: the product is one
    size_t st = 0;
    size_t ms = 0;         // 2 rows of 2 n + 1 scalars: r_i | t_i = r_i z_i | -u, then 0 | r_i | 0 (the second sum over the same points)
    size_t mp = 0, minf = 0;    // 2 n + 1 points C_i | pi_i | g1, + infinity bytes
    size_t part = 0, sum = 0;   // the fold's partial accumulators (zkp_groth16_plan.hpp, fold_plan(n, 1)): sizes passed in
    size_t u = 0;          // u = sum r_i y_i
    size_t mg1 = 0, minf1 = 0;  // the two G1 sums + infinity bytes
    size_t mg2 = 0;        // -g2, [tau]g2
    size_t ml = 0;         // ML_RECORDS Fp12 records
    size_t total = 0;
};
// n >= 1 and !args_bad(n, flags); part_bytes / sum_bytes: the fold's partial regions for (n, 1)
inline Layout make_layout(size_t n, int flags, size_t part_bytes, size_t sum_bytes) {
    Layout L;
    L.n_status = ((flags & POINTS_CHECKED) ? 0 : 2 * n) + ((flags & VK_CHECKED) ? 0 : 3);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    L.flag = take(2 * sizeof(int32_t));
    L.st = take(L.n_status);
    L.ms = take(2 * (2 * n + 1) * 32);
    L.mp = take((2 * n + 1) * 96);
    L.minf = take(2 * n + 1);
    L.part = take(part_bytes);
    L.sum = take(sum_bytes);
    L.u = take(32);
    L.mg1 = take(2 * 96);
    L.minf1 = take(2);
    L.mg2 = take(2 * 192);
    L.ml = take(ML_RECORDS * 576);
    L.total = o;
    return L;
}

}  // namespace kzg
}  // namespace zkp
