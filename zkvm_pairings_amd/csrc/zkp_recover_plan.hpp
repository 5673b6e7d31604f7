// zkp_recover_plan.hpp -- the PURE host arithmetic of the cell recovery (zkp_das_recover_batch): the argument limits, the shape of a
// call, the column kernel's tile, the slice length and the layout of the workspace.  No HIP type, no allocation, no I/O.
// zkp_recover.hip compiles this text for the device; tests/recover_plan_check.cpp compiles it with g++ -fsanitize=address,undefined
// and walks it at the ABI's maxima.
//
// A blob: N = 2^log2_n coefficients, cells of l = 2^log2_l values, D = 2 N points, M = D / l = 2^mu cells, k = M / 2.  Column i < l of
// the cells' interpolants is a Reed-Solomon codeword of length M: the column kernel keeps whole columns in a tile of 2^10 elements
// (32 KiB of LDS, zkp_poly_plan.hpp's tile), 2^cl = 2^(10 - mu) column slots of M positions each, tile element e = c | (p << cl).  A
// workgroup takes C = min(l, 2^cl) consecutive columns of one blob; the other slots hold zeros.  C >= 4 (runs of 128 B) whenever
// l >= 4 and M <= 256; M = 512 and M = 1024 leave two columns and one.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zkp_kzg_plan.hpp"
#include "zkp_poly_plan.hpp"

namespace zkp {
namespace rec {

constexpr unsigned MAX_LOG2_N = 19;
constexpr unsigned MAX_LOG2_M = poly::COSET_LOG2;      // a column fits the tile, and 7^t comes from the low coset table alone
constexpr size_t MAX_TOTAL = (size_t)1 << 26;          // n * D
constexpr size_t SLICE_POINTS = (size_t)1 << 21;       // points of one slice: 64 MiB of interpolant coefficients
constexpr int ALL_FLAGS = poly::NTT_BITREV;
static_assert(MAX_LOG2_M == poly::TILE_LOG2, "the tile holds one column of the largest M");

constexpr bool args_bad(size_t n, unsigned log2_n, unsigned log2_l, int flags) {
    return log2_n > MAX_LOG2_N || log2_l > log2_n || log2_n + 1 - log2_l > MAX_LOG2_M || (flags & ~ALL_FLAGS) || n > (MAX_TOTAL >> (log2_n + 1));
}

struct Shape {
    unsigned log2_d = 0, mu = 0, cl = 0;   // D = 2^log2_d, M = 2^mu, 2^cl column slots in a tile
    uint32_t cols = 0;                     // C: columns a workgroup works on
    uint32_t groups = 0;                   // workgroups of a blob: l / C
};
// !args_bad
inline Shape shape_of(unsigned log2_n, unsigned log2_l) {
    Shape s;
    s.log2_d = log2_n + 1;
    s.mu = s.log2_d - log2_l;
    s.cl = poly::TILE_LOG2 - s.mu;
    const unsigned c_log2 = log2_l < s.cl ? log2_l : s.cl;
    s.cols = 1u << c_log2;
    s.groups = 1u << (log2_l - c_log2);
    return s;
}

// slices of whole blobs: at most SLICE_POINTS points each, and at least one blob
constexpr size_t slice_of(size_t n, unsigned log2_n) {
    const size_t per = (SLICE_POINTS >> (log2_n + 1)) ? (SLICE_POINTS >> (log2_n + 1)) : 1;
    return n < per ? n : per;
}

// the regions of the kzg workspace for slices of `slice` blobs, every one 256-byte aligned
struct Layout {
    size_t slice = 0;
    size_t coef = 0;     // slice x M x l interpolant coefficients (none for l = 1: the values are the coefficients)
    size_t ntt = 0;      // the workspace of the size-l transform (natural order above 2^10 only)
    size_t zc = 0;       // slice x M coefficients of Z
    size_t zr = 0;       // Z on the M-th roots
    size_t zs = 0;       // Z on the coset 7 w_M^t, then its inverses
    size_t total = 0;
};
// n >= 1 and !args_bad
inline Layout layout(size_t n, unsigned log2_n, unsigned log2_l, int flags) {
    Layout L;
    const Shape s = shape_of(log2_n, log2_l);
    L.slice = slice_of(n, log2_n);
    const size_t cells = L.slice << s.mu;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += kzg::align256(bytes); return at; };
    L.coef = take(log2_l ? (L.slice << s.log2_d) * 32 : 0);
    L.ntt = take(log2_l ? poly::ntt_workspace_bytes(cells, log2_l, poly::NTT_INVERSE | (flags & poly::NTT_BITREV)) : 0);
    L.zc = take(cells * 32);
    L.zr = take(cells * 32);
    L.zs = take(cells * 32);
    L.total = o;
    return L;
}

// what the column kernel receives by value
struct Column {
    uint32_t log2_l = 0, mu = 0, cl = 0, cols = 0, groups = 0, bitrev = 0;
    uint32_t log2_d = 0;
    uint32_t tshift_d = 0;    // w_D^x is entry x << tshift_d of the domain table
    uint32_t tshift_m = 0;    // w_M^x is entry x << tshift_m
};
inline Column column_of(unsigned log2_n, unsigned log2_l, int flags, unsigned table_log2) {
    const Shape s = shape_of(log2_n, log2_l);
    Column a;
    a.log2_l = log2_l;
    a.mu = s.mu;
    a.cl = s.cl;
    a.cols = s.cols;
    a.groups = s.groups;
    a.bitrev = (flags & poly::NTT_BITREV) ? 1 : 0;
    a.log2_d = s.log2_d;
    a.tshift_d = table_log2 - s.log2_d;
    a.tshift_m = table_log2 - s.mu;
    return a;
}

// ---- the column kernel's index arithmetic ------------------------------------------------------------------------------------------
// the rounds of a transform over the mu position bits of the tile: zkp_poly_plan.hpp's rounds of a pass with cl companions below
ZKP_POLY_HD poly::Pass pass_of(uint32_t mu, uint32_t cl, uint32_t dit) {
    poly::Pass p;
    p.k = mu;
    p.t = poly::TILE_LOG2;
    p.lo = 0;
    p.kp = mu;
    p.cl = cl;
    p.ch = 0;
    p.dit = dit;
    return p;
}
// the twiddle of the butterfly on tile bit b whose upper element is tile element e: an exponent of w_M (0: one)
ZKP_POLY_HD uint32_t twiddle_exp(uint32_t mu, uint32_t cl, uint32_t e, uint32_t b, uint32_t inverse) {
    const uint32_t p = b - cl, i = e >> cl;
    const uint32_t ex = (i & poly::low_mask(p)) << (mu - 1 - p);
    return inverse ? ((1u << mu) - ex) & poly::low_mask(mu) : ex;
}
// c_m^-i = w_D^(-(m' i) mod D): the exponent (zkp_cells_plan.hpp's inverse_power_index)
ZKP_POLY_HD uint32_t inverse_power(uint32_t mp, uint32_t i, uint32_t log2_d) {
    const uint32_t mask = poly::low_mask(log2_d);
    return ((1u << log2_d) - (uint32_t)(((uint64_t)mp * i) & mask)) & mask;
}

}  // namespace rec
}  // namespace zkp
