// zkp_rlc_plan.hpp -- the host side's PURE arithmetic of the random-linear-combination batch check (zkp_pairing_check_batch_rlc):
// the argument limits, the scalar r = a + b z^2 of one check, how many columns one MSM call takes and the layout of the workspace.
// No HIP type, no allocation, no I/O: included by zkp_rlc.hip (the product) and compiled with g++ -fsanitize=address,undefined by
// tests/test_rlc_cpu.py, which walks it over the sizes the C ABI admits.
//
// Shape: n checks; check c is the product of k free pairs, s2 pairs (col_g1[c][j], fixed_g2[j]) and s1 pairs (fixed_g1[j], col_g2[c][j]).
// Column j of the s2 ones becomes ONE pair (sum_c [r_c] col_g1[c][j], fixed_g2[j]) through a G1 MSM of n terms, likewise for s1 with G2.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZKP_RLC_HD __host__ __device__
#else
#define ZKP_RLC_HD
#endif

namespace zkp {
namespace rlc {

constexpr size_t MAX_COL_TERMS = (size_t)1 << 24;   // checks a column may sum (the MSM's m * n_msm limit, one column per call at most)
constexpr size_t MAX_COLS = 0xffff;                 // s1, s2 (as k)
constexpr size_t MAX_PAIRS = 0x7fffffff;            // n * k (zkp_plan.hpp's too_many)
// z^2 for the BLS parameter z = 0xd201000000010000 (|z|; the sign drops out of the square), low word first
constexpr uint64_t Z2_LO = 0x0000000100000000ull, Z2_HI = 0xac45a4010001a402ull;
constexpr size_t SCALAR_U64 = 4;                    // an MSM scalar: 4 u64, the value below 2^192
constexpr size_t ML_RECORDS = 3;                    // Miller values of the free pairs and of the column pairs, then Gt

// the sizes a call may carry; pointer checks are the entry point's
constexpr bool args_bad(size_t n, size_t k, size_t s1, size_t s2) {
    return n > MAX_PAIRS || k > MAX_COLS || s1 > MAX_COLS || s2 > MAX_COLS || (k && n > MAX_PAIRS / k) ||
           ((s1 || s2) && n > MAX_COL_TERMS) || (n && !k && !s1 && !s2);
}

// r = a + b z^2 as a 4-word integer (< 2^192): distinct for distinct (a, b) since a < 2^64 < z^2, and below r (the group order) since
// (2^64 - 1)(1 + z^2) < r - so every r_c is a nonzero exponent unless a = b = 0
ZKP_RLC_HD inline void scalar(uint64_t a, uint64_t b, uint64_t* out) {
    const unsigned __int128 lo = (unsigned __int128)b * Z2_LO + a;
    const unsigned __int128 hi = (unsigned __int128)b * Z2_HI + (uint64_t)(lo >> 64);
    out[0] = (uint64_t)lo;
    out[1] = (uint64_t)hi;
    out[2] = (uint64_t)(hi >> 64);
    out[3] = 0;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    size_t cols = 0;        // columns per MSM call: every one of them sums n terms, cols * n <= MAX_COL_TERMS
    size_t n_status = 0;    // status bytes of the points check (0 with ZKP_RLC_POINTS_CHECKED)
    // byte offsets into the workspace, every region 256-byte aligned
    size_t flag = 0;        // int32 [0]: every point valid and no zero scalar, [1]: the product is one
    size_t st = 0;          // status bytes: free G1, free G2, col_g1, fixed_g2, col_g2, fixed_g1
    size_t sc = 0;          // the n scalars, `cols` copies (the MSM reads one row of n per sum)
    size_t sg1 = 0, sinf = 0;          // scaled free G1 points + infinity bytes (n k)
    size_t tg1 = 0, tinf1 = 0;         // col_g1 column-major (s2 rows of n) + infinity bytes
    size_t tg2 = 0, tinf2 = 0;         // col_g2 column-major (s1 rows of n)
    size_t mg1 = 0, mg2 = 0, minf1 = 0, minf2 = 0;   // the s2 + s1 column pairs: MSM sums and fixed points
    size_t ml = 0;          // ML_RECORDS Fp12 records
    size_t total = 0;
};

// n >= 1 and !args_bad(n, k, s1, s2)
inline Layout make_layout(size_t n, size_t k, size_t s1, size_t s2, bool check) {
    Layout L;
    const size_t smax = s1 > s2 ? s1 : s2, fit = MAX_COL_TERMS / n;
    L.cols = smax < fit ? smax : fit;
    L.n_status = check ? 2 * n * k + (n + 1) * (s1 + s2) : 0;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    L.flag = take(2 * sizeof(int32_t));
    L.st = take(L.n_status);
    L.sc = take(L.cols * n * SCALAR_U64 * 8);
    L.sg1 = take(n * k * 96);
    L.sinf = take(n * k);
    L.tg1 = take(n * s2 * 96);
    L.tinf1 = take(n * s2);
    L.tg2 = take(n * s1 * 192);
    L.tinf2 = take(n * s1);
    L.mg1 = take((s1 + s2) * 96);
    L.mg2 = take((s1 + s2) * 192);
    L.minf1 = take(s1 + s2);
    L.minf2 = take(s1 + s2);
    L.ml = take(ML_RECORDS * 576);
    L.total = o;
    return L;
}

}  // namespace rlc
}  // namespace zkp
