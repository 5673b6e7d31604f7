// zkp_groth16_plan.hpp -- the host side's PURE arithmetic of the Fr fold (zkp_fr_fold_batch) and of the batched Groth16 verifier
// (zkp_groth16_verify_batch): the argument limits, the grid of the fold and the layout of the workspace.  No HIP type, no allocation,
// no I/O: included by zkp_groth16.hip and zkp_pairings.hip (the product) and compiled with g++ -fsanitize=address,undefined by
// tests/test_groth16_cpu.py, which walks it over the sizes the C ABI admits.
//
// Shape: n proofs (A_c, B_c, C_c) with l public inputs each, one key (alpha, beta, gamma, delta, IC_0 .. IC_l).  The verifier's own
// regions live here, beside the RLC workspace (zkp_rlc_plan.hpp), never inside it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkp {
namespace g16 {

constexpr size_t MAX_PROOFS = (size_t)1 << 24;   // n: the C column is one MSM of n terms (the MSM's limit), and the fold's accumulator bound
constexpr size_t MAX_INPUTS = 0xffff;            // l
constexpr size_t MAX_TERMS = 0x7fffffff;         // n * l
constexpr size_t ACC_BYTES = 17 * 4;             // one accumulator of the fold (zkp_fr.hpp: ACC_WORDS)
constexpr unsigned FOLD_TPB = 256;               // threads of a fold workgroup: tw lanes along i times FOLD_TPB / tw rows
constexpr unsigned FOLD_MAX_TW = 64;
constexpr unsigned FOLD_BLOCKS = 1024;           // workgroups the fold aims at (four per compute unit of an MI355X)
constexpr size_t ML_RECORDS = 3;                 // Miller values of the free pairs and of the three folded pairs, then Gt
constexpr size_t FOLDED_PAIRS = 3;               // (sum [r_c] C_c, -delta), (sum [s_i] IC_i, -gamma), ([s_0] alpha, -beta)

constexpr bool fold_args_bad(size_t n, size_t l) { return n > MAX_PROOFS || l > MAX_INPUTS || (l && n > MAX_TERMS / l); }

// the fold's grid: a workgroup covers tw consecutive i of `rows` rows at a time and strides over c; `parts` workgroups share a tile of i
// and leave one partial accumulator per i each, `sum_parts` workgroups do the same for the plain sum of the weights
struct FoldPlan {
    unsigned tw = 1, rows = FOLD_TPB, tiles = 0, parts = 0, sum_parts = 0;
    size_t part_bytes = 0, sum_bytes = 0;
};
// n >= 1 and !fold_args_bad(n, l)
inline FoldPlan fold_plan(size_t n, size_t l) {
    FoldPlan p;
    while (p.tw < l && p.tw < FOLD_MAX_TW) p.tw <<= 1;
    p.rows = FOLD_TPB / p.tw;
    p.tiles = (unsigned)((l + p.tw - 1) / p.tw);
    if (l) {
        const size_t need = (n + p.rows - 1) / p.rows, aim = FOLD_BLOCKS / p.tiles ? FOLD_BLOCKS / p.tiles : 1;
        p.parts = (unsigned)(need < aim ? need : aim);
    }
    const size_t sneed = (n + FOLD_TPB - 1) / FOLD_TPB;
    p.sum_parts = (unsigned)(sneed < FOLD_BLOCKS ? sneed : FOLD_BLOCKS);
    p.part_bytes = (size_t)p.parts * l * ACC_BYTES;
    p.sum_bytes = (size_t)p.sum_parts * ACC_BYTES;
    return p;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the workspace of a bare zkp_fr_fold_batch[_dev]: the two partial regions
struct FoldLayout { size_t part = 0, sum = 0, total = 0; };
inline FoldLayout fold_layout(const FoldPlan& p) {
    FoldLayout L;
    L.part = 0;
    L.sum = align256(p.part_bytes);
    L.total = L.sum + align256(p.sum_bytes);
    return L;
}

// flags of zkp_groth16_verify_batch (the header's ZKP_GROTH16_*)
constexpr int POINTS_CHECKED = 1, VK_CHECKED = 2, ALL_FLAGS = 3;

constexpr bool args_bad(size_t n, size_t l, int flags) { return fold_args_bad(n, l) || (flags & ~ALL_FLAGS); }

struct Layout {
    size_t n_status = 0;    // status bytes of the points check: A, B, C (3 n) unless POINTS_CHECKED; alpha, IC_0 .. IC_l, then -delta, -gamma,
                            // -beta (l + 5) unless VK_CHECKED
    // byte offsets into the workspace, every region 256-byte aligned
    size_t flag = 0;        // int32 [0]: every point valid, every input < r, no zero (a, b); [1]: the product is one
    size_t st = 0;
    size_t sc = 0;          // r_c = a_c + b_c z^2, n x 32 B: the C column's MSM scalars and the fold's weights
    size_t sg1 = 0, sinf = 0;    // [r_c] A_c + infinity bytes
    size_t part = 0, sum = 0;    // the fold's partial accumulators (FoldPlan)
    size_t ms = 0;          // 2 (l + 1) scalars: s_0 .. s_l, then s_0 and l zeros (the second sum of the small MSM is [s_0] alpha)
    size_t mp = 0;          // 2 (l + 1) G1 points: IC_0 .. IC_l, then alpha, IC_1 .. IC_l
    size_t mg1 = 0, minf1 = 0;   // the three G1 sums, in FOLDED_PAIRS order, + infinity bytes
    size_t mg2 = 0;         // -delta, -gamma, -beta
    size_t ml = 0;          // ML_RECORDS Fp12 records
    size_t total = 0;
};

// n >= 1 and !args_bad(n, l, flags)
inline Layout make_layout(size_t n, size_t l, int flags) {
    Layout L;
    const FoldPlan fp = fold_plan(n, l);
    L.n_status = ((flags & POINTS_CHECKED) ? 0 : 3 * n) + ((flags & VK_CHECKED) ? 0 : l + 2 + FOLDED_PAIRS);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    L.flag = take(2 * sizeof(int32_t));
    L.st = take(L.n_status);
    L.sc = take(n * 32);
    L.sg1 = take(n * 96);
    L.sinf = take(n);
    L.part = take(fp.part_bytes);
    L.sum = take(fp.sum_bytes);
    L.ms = take(2 * (l + 1) * 32);
    L.mp = take(2 * (l + 1) * 96);
    L.mg1 = take(FOLDED_PAIRS * 96);
    L.minf1 = take(FOLDED_PAIRS);
    L.mg2 = take(FOLDED_PAIRS * 192);
    L.ml = take(ML_RECORDS * 576);
    L.total = o;
    return L;
}

}  // namespace g16
}  // namespace zkp
