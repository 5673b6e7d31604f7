// zkp_cells_plan.hpp -- the PURE arithmetic of the KZG cell proofs (zkp_kzg_cells_setup, zkp_kzg_cells_batch): the argument limits, the
// sizes of a shape, the source maps of the setup vectors and of the coefficient vectors, the lanes of the multiply-accumulate and of the
// sum of its partials, the group size g, the slices and the workspace.  The transforms themselves are zkp_fk20_plan.hpp's.  No HIP type,
// no allocation, no I/O.  zkp_coop.hip and zkp_cells.hip compile this text for the device; tests/cells_plan_check.cpp compiles it with
// g++ -fsanitize=address,undefined and walks it at the ABI's maxima.
#pragma once
#include "zkp_fk20_plan.hpp"

namespace zkp {
namespace cells {

constexpr unsigned CELLS_MAX_LOG2 = fk20::FK20_MAX_LOG2;      // N <= 2^19
constexpr size_t CELLS_MAX_TOTAL = fk20::FK20_MAX_TOTAL;      // n * N <= 2^21
constexpr int CELLS_ALL_FLAGS = fk20::NTT_BITREV;
constexpr unsigned G_MAX_LOG2 = 2;                            // g <= 4: see group_log2
constexpr size_t FULL_LANES = (size_t)1 << 16;                // one wavefront on every SIMD of 256 compute units

constexpr bool setup_args_bad(unsigned log2_n, unsigned log2_l) { return log2_n > CELLS_MAX_LOG2 || log2_l > log2_n; }
constexpr bool cells_args_bad(size_t n, unsigned log2_n, unsigned log2_l, unsigned log2_ext, int flags) {
    return log2_n > CELLS_MAX_LOG2 || log2_l > log2_n || log2_ext > 1 || (flags & ~CELLS_ALL_FLAGS) || n > (CELLS_MAX_TOTAL >> log2_n);
}

// the sizes of a shape, as logarithms: k = N / l vectors entries, transforms of 2 k, M = e k proofs, a block of 2 M records per polynomial
// (the inverse transform of size 2 k runs in its lower half or in all of it, the forward one of size M in its upper half)
struct Shape {
    uint32_t n = 0, l = 0, k = 0, k1 = 0, m = 0, blk = 0;
};
ZKP_FK20_HD Shape shape_of(unsigned log2_n, unsigned log2_l, unsigned log2_ext) {
    Shape s;
    s.n = log2_n;
    s.l = log2_l;
    s.k = log2_n - log2_l;
    s.k1 = s.k + 1;
    s.m = s.k + log2_ext;
    s.blk = s.m + 1;
    return s;
}

// ---- step 1: entry t < 2 k of c_i = (f_{N-1-i}, 0 x (k + 1), f_{2l-1-i}, .., f_{N-l-1-i}): the coefficient's index, or -1 for zero.
// It is fk20::coeff_source of g_d = f_{(d+1) l - 1 - i}, d < k
ZKP_FK20_HD int64_t coeff_source(uint32_t t, uint32_t i, uint32_t log2_k, uint32_t log2_l) {
    const int64_t d = fk20::coeff_source(t, log2_k);
    return d < 0 ? -1 : (((d + 1) << log2_l) - 1 - (int64_t)i);
}

// ---- step 3.  Lane -> (polynomial j, slot t < 2 k, group q < l / g of g = 2^s consecutive strides).  The scalar of stride i is element
// ((j l + i) << k1) + t of the transformed vectors; its base is point (i << k1) + bitrev(t) of the setup; the lane's partial is record
// (lane index) of the partials, or - when g = l - record (j << blk) + t of the blocks
struct Mac {
    uint32_t log2_l = 0, k1 = 0, blk = 0, s = 0;
    uint32_t n_lane = 0;     // n_poly << (k1 + log2_l - s)
};
ZKP_FK20_HD void mac_lane(const Mac& a, uint32_t lane, uint32_t* j, uint32_t* t, uint32_t* i0) {
    const uint32_t gl = a.log2_l - a.s;                       // log2 of the groups of a slot
    *i0 = (lane & fk20::low_mask(gl)) << a.s;
    *t = (lane >> gl) & fk20::low_mask(a.k1);
    *j = lane >> (gl + a.k1);
}
ZKP_FK20_HD uint64_t mac_scalar(const Mac& a, uint32_t j, uint32_t t, uint32_t i) { return ((((uint64_t)j << a.log2_l) + i) << a.k1) + t; }
ZKP_FK20_HD uint32_t mac_base(const Mac& a, uint32_t t, uint32_t i) { return (i << a.k1) + fk20::bitrev(t, a.k1); }
// the LDS of a workgroup of k_cell_mac: x and y of g bases, four quads of 16 B per lane each
constexpr uint32_t mac_lds_bytes(uint32_t s) { return (2u << s) * 4 * 64 * 16; }
ZKP_FK20_HD uint32_t mac_record(const Mac& a, uint32_t j, uint32_t t) { return (j << a.blk) + t; }
// the sum: lane -> (j, t); its l / g partials are consecutive, from (lane << (log2_l - s))
struct Sum {
    uint32_t log2_l = 0, k1 = 0, blk = 0, s = 0;
    uint32_t n_lane = 0;     // n_poly << k1
};

// ---- the group size.  A lane's chain is 255 doublings and 255 g additions; the launch has lanes1 / g lanes, lanes1 = 2 N polynomials.  Up
// to FULL_LANES lanes every lane has a SIMD's issue slot to itself, so the shortest chain wins: g = 1.  Beyond that the launch's time goes
// with its total work, lanes1 (255 / g doublings + 255 additions): the smallest g that brings the lanes back to FULL_LANES, never above l.
// A slice holds at most 2^18 scalars (or one polynomial), so g = 4 is the largest value that rule asks for below N = 2^18; the additions
// that remain are 255 per base whatever g is, and at g = 4 the doublings are down to a sixth of them.
ZKP_FK20_HD uint32_t group_log2(size_t n_poly, unsigned log2_n, unsigned log2_l) {
    const size_t lanes1 = n_poly << (log2_n + 1);
    uint32_t s = 0;
    while (s < G_MAX_LOG2 && s < log2_l && (lanes1 >> s) > FULL_LANES) s++;
    return s;
}

// ---- slices of whole polynomials, floor(2^17 / N) each (at least one), FK20's; per polynomial of a slice 2 N field elements, 2 M records
// and - unless g = l - 2 N / g partial records
struct Layout {
    size_t slice = 0;
    uint32_t s = 0;          // log2 g of every slice of the call
    size_t rec = 0, part = 0, fr = 0, total = 0;
};
constexpr size_t slice_polys(size_t n, unsigned log2_n) { return fk20::slice_vectors(n, log2_n + 1); }
ZKP_FK20_HD Layout layout(size_t n, unsigned log2_n, unsigned log2_l, unsigned log2_ext) {
    Layout L;
    const Shape sh = shape_of(log2_n, log2_l, log2_ext);
    L.slice = slice_polys(n, log2_n);
    L.s = group_log2(L.slice, log2_n, log2_l);
    L.rec = 0;
    L.part = fk20::up256((L.slice << sh.blk) * fk20::REC_BYTES);
    const size_t parts = L.s == log2_l ? 0 : (L.slice << (log2_n + 1)) >> L.s;
    L.fr = L.part + fk20::up256(parts * fk20::REC_BYTES);
    L.total = L.fr + fk20::up256((L.slice << (log2_n + 1)) * 32);
    return L;
}
// the setup runs its l transforms of size 2 k as one launch sequence: 2 N records
constexpr size_t setup_workspace_bytes(unsigned log2_n) { return ((size_t)2 << log2_n) * fk20::REC_BYTES; }

// ---- the verifier (zkp_kzg_cell_verify_batch).  Its limits are those of the calls it composes: the Fr transform and the domain table
// (log2_d <= 20, n l <= 2^26), the fold's width (l <= 0xffff: log2_l <= 15), the two-row MSM over 2 n + l points (2 (2 n + l) <= 2^24)
constexpr unsigned VERIFY_MAX_LOG2_D = 20, VERIFY_MAX_LOG2_L = 15;
constexpr size_t VERIFY_MAX_CELLS = (size_t)1 << 21, VERIFY_MAX_VALUES = (size_t)1 << 26;
constexpr int VERIFY_POINTS_CHECKED = 4, VERIFY_VK_CHECKED = 8, VERIFY_ALL_FLAGS = fk20::NTT_BITREV | 4 | 8;
constexpr bool verify_args_bad(size_t n, unsigned log2_d, unsigned log2_l, int flags) {
    return log2_d > VERIFY_MAX_LOG2_D || log2_l > log2_d || log2_l > VERIFY_MAX_LOG2_L || (flags & ~VERIFY_ALL_FLAGS) || n > VERIFY_MAX_CELLS ||
           n > (VERIFY_MAX_VALUES >> log2_l);
}
// (-(m i) mod D): the index of c^-i = w_D^-(m i) in the domain table of D = 2^log2_d points, m < D, i < D
ZKP_FK20_HD uint32_t inverse_power_index(uint32_t m, uint32_t i, uint32_t log2_d) {
    const uint32_t mask = fk20::low_mask(log2_d);
    return (0u - (uint32_t)(((uint64_t)m * i) & mask)) & mask;
}
struct VerifyLayout {
    size_t n_status = 0;   // status bytes of the points check: C and pi (2 n) unless POINTS_CHECKED; the l monomial points, -g2, [tau^l]g2 unless VK_CHECKED
    // byte offsets, every region 256-byte aligned
    size_t flag = 0;       // int32 [0]: every point valid, every value < r, every index < M, no zero (a, b); [1]: the product is one
    size_t st = 0;
    size_t coef = 0;       // n x l coefficients of the interpolants
    size_t ntt = 0;        // the Fr transform's workspace (natural order above its tile only): size passed in
    size_t ms = 0;         // 2 rows of 2 n + l scalars: r_j | r_j c_j^l | -a_i, then 0 | r_j | 0
    size_t mp = 0, minf = 0;    // 2 n + l points C_j | pi_j | monomial, + infinity bytes
    size_t part = 0;       // the fold's partial accumulators (zkp_groth16_plan.hpp, fold_plan(n, l)): size passed in
    size_t a = 0;          // a_i = sum_j r_j coef[j][i]
    size_t mg1 = 0, minf1 = 0, mg2 = 0, ml = 0;   // the two G1 sums + infinity bytes; -g2, [tau^l]g2; two Fp12 records
    size_t total = 0;
};
// n >= 1 and !verify_args_bad
inline VerifyLayout verify_layout(size_t n, unsigned log2_l, int flags, size_t ntt_bytes, size_t part_bytes) {
    VerifyLayout L;
    const size_t l = (size_t)1 << log2_l, m = 2 * n + l;
    L.n_status = ((flags & VERIFY_POINTS_CHECKED) ? 0 : 2 * n) + ((flags & VERIFY_VK_CHECKED) ? 0 : l + 2);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += fk20::up256(bytes); return at; };
    L.flag = take(2 * sizeof(int32_t));
    L.st = take(L.n_status);
    L.coef = take(n * l * 32);
    L.ntt = take(ntt_bytes);
    L.ms = take(2 * m * 32);
    L.mp = take(m * 96);
    L.minf = take(m);
    L.part = take(part_bytes);
    L.a = take(l * 32);
    L.mg1 = take(2 * 96);
    L.minf1 = take(2);
    L.mg2 = take(2 * 192);
    L.ml = take(2 * 576);
    L.total = o;
    return L;
}

}  // namespace cells
}  // namespace zkp
