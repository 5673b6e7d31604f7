// zkp_fk20_plan.hpp -- the PURE arithmetic of the G1 NTT (zkp_g1_ntt_batch) and of the FK20 proofs (zkp_kzg_fk20_setup, zkp_kzg_fk20_batch):
// the argument limits, the slices, grids and workspace bytes, the records a butterfly lane touches and its twiddle, the source maps of
// the first stage (wire order, the FK20 setup vector, the lower half of a 2N block), the coefficient vector c of a polynomial, and the
// split of a scalar at z^2.  No HIP type, no allocation, no I/O.  zkp_coop.hip and zkp_fk20.hip compile this text for the device;
// tests/fk20_plan_check.cpp compiles it with g++ -fsanitize=address,undefined and walks it at the ABI's maxima.
//
// The transform.  Decimation in time only: position i of the workspace takes input bitrev(i), stage p = 0 .. k - 1 pairs the records whose
// positions differ in bit p - A' = A + [w^t] B, B' = A - [w^t] B with t = (i mod 2^p) << (k - 1 - p), N - t for the inverse - and leaves
// natural order.  Stage 0 multiplies nothing.  The first stage reads its two inputs wherever the caller's order puts them and the last
// kernel stores wherever the caller's order wants them, so neither order costs a pass:
//   forward            load bitrev, store natural          forward, BITREV    load bitrev, store bitrev
//   inverse            load bitrev, store natural          inverse, BITREV    load natural (slot i IS w^bitrev(i)), store natural
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZKP_FK20_HD __host__ __device__ __forceinline__
#define ZKP_FK20_UNROLL _Pragma("unroll")
#define ZKP_FK20_NOUNROLL _Pragma("unroll 1")
#else
#define ZKP_FK20_HD inline
#define ZKP_FK20_UNROLL
#define ZKP_FK20_NOUNROLL
#endif

namespace zkp {
namespace fk20 {

constexpr unsigned G1NTT_MAX_LOG2 = 20;
constexpr size_t G1NTT_MAX_TOTAL = (size_t)1 << 22;      // n_vec * N
constexpr size_t SLICE_POINTS = (size_t)1 << 18;         // points of one slice (a single vector may be larger)
constexpr unsigned FK20_MAX_LOG2 = 19;                   // the transforms are of size 2 N
constexpr size_t FK20_MAX_TOTAL = (size_t)1 << 21;       // n * N
constexpr int NTT_INVERSE = 1, NTT_BITREV = 2, G1NTT_ALL_FLAGS = 3, FK20_ALL_FLAGS = 2;
constexpr size_t REC_BYTES = 192;                        // a Jacobian record: three 64-byte field records
constexpr size_t SPLIT_BYTES = 32;                       // a split twiddle: a, b of 128 bits each
constexpr unsigned LANES = 64;                           // one wavefront per workgroup, one lane per butterfly

constexpr bool g1ntt_args_bad(size_t n_vec, unsigned log2_n, int flags) {
    return log2_n > G1NTT_MAX_LOG2 || (flags & ~G1NTT_ALL_FLAGS) || n_vec > (G1NTT_MAX_TOTAL >> log2_n);
}
constexpr bool setup_args_bad(unsigned log2_n) { return log2_n > FK20_MAX_LOG2; }
constexpr bool fk20_args_bad(size_t n, unsigned log2_n, int flags) {
    return log2_n > FK20_MAX_LOG2 || (flags & ~FK20_ALL_FLAGS) || n > (FK20_MAX_TOTAL >> log2_n);
}
// whole vectors of 2^log2_len points per slice: at most SLICE_POINTS points, and at least one vector
constexpr size_t slice_vectors(size_t n_vec, unsigned log2_len) {
    const size_t per = (SLICE_POINTS >> log2_len) ? (SLICE_POINTS >> log2_len) : 1;
    return n_vec < per ? n_vec : per;
}
constexpr size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
// the G1 NTT's workspace: one record per point of a slice.  At most max(2^18, N) records: 48 MiB up to N = 2^18, 192 MiB at N = 2^20
constexpr size_t g1ntt_workspace_bytes(size_t n_vec, unsigned log2_n) { return (slice_vectors(n_vec, log2_n) << log2_n) * REC_BYTES; }
// FK20: a slice of polynomials holds 2 N records and 2 N field elements each.  At most max(2^18, 2 N) of either: 56 MiB up to N = 2^17,
// 224 MiB at N = 2^19
struct Fk20Layout {
    size_t slice = 0;      // polynomials per slice
    size_t rec = 0, fr = 0, total = 0;
};
constexpr Fk20Layout fk20_layout(size_t n, unsigned log2_n) {
    Fk20Layout L;
    L.slice = slice_vectors(n, log2_n + 1);
    const size_t pts = L.slice << (log2_n + 1);
    L.rec = 0;
    L.fr = up256(pts * REC_BYTES);
    L.total = L.fr + up256(pts * 32);
    return L;
}
constexpr size_t split_table_bytes(unsigned log2_n) { return SPLIT_BYTES << log2_n; }
// workgroups of LANES lanes for `items` lanes; every count of a launch stays in 32 bits: items <= 2^22 here
constexpr uint32_t grid(size_t items) { return (uint32_t)((items + LANES - 1) / LANES); }
constexpr bool count_ok(size_t items) { return items <= ((size_t)1 << 22); }

ZKP_FK20_HD uint32_t low_mask(unsigned bits) { return bits >= 32 ? 0xffffffffu : (1u << bits) - 1u; }
ZKP_FK20_HD uint32_t bitrev(uint32_t v, unsigned bits) {
    if (!bits) return 0;
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - bits);
}

// where the transforms of a launch live: vector j's position e is record (j << vs_log2) + off + e
struct Span {
    uint32_t k = 0;          // log2 of the transform
    uint32_t vs_log2 = 0;    // log2 of the distance between two vectors, in records (>= k)
    uint32_t off = 0;        // first record of a vector inside its block
    uint32_t n_vec = 0;
};
ZKP_FK20_HD uint32_t span_record(const Span& a, uint32_t j, uint32_t e) { return (j << a.vs_log2) + a.off + e; }

// ---- a twiddled stage -----------------------------------------------------------------------------------------------------------------
struct Stage {
    Span at;
    uint32_t p = 0;          // the stage's bit, 1 <= p < k
    uint32_t inverse = 0;
    uint32_t tshift = 0;     // split table log2 - k: entry t of this transform's domain is table[t << tshift]
    uint32_t n_bfly = 0;     // n_vec << (k - 1)
};
// lane t < n_bfly -> the two records of its butterfly and the index of its twiddle in the split table
ZKP_FK20_HD void stage_lane(const Stage& s, uint32_t t, uint32_t* r0, uint32_t* r1, uint32_t* tw) {
    const uint32_t k = s.at.k, j = t >> (k - 1), b = t & low_mask(k - 1);
    const uint32_t i0 = ((b >> s.p) << (s.p + 1)) | (b & low_mask(s.p));
    const uint32_t ex = (i0 & low_mask(s.p)) << (k - 1 - s.p);
    *r0 = span_record(s.at, j, i0);
    *r1 = span_record(s.at, j, i0 | (1u << s.p));
    *tw = (s.inverse ? ((1u << k) - ex) & low_mask(k) : ex) << s.tshift;
}

// ---- the first stage (bit 0, twiddle one): where position e of vector j comes from -------------------------------------------------------
enum { SRC_WIRE = 0, SRC_SETUP = 1, SRC_REC = 2, SRC_CELLS = 3 };
struct First {
    Span at;                 // where the records go
    uint32_t mode = SRC_WIRE;
    uint32_t perm = 0;       // position e takes input bitrev(e)
    uint32_t src_off = 0;    // SRC_REC: first record of the source vector inside its block
    uint32_t src_len = 0;    // SRC_REC: inputs from src_len on are the identity, whatever their records hold (0: every input is a record).
                             // PRECONDITION: perm set and src_len >= 2^(k - 1) (or k = 0), so that input A of every butterfly - bitrev of an
                             // even position, below 2^(k - 1) - is a record: k_g1ntt_first<SRC_REC> reads A without testing it
    uint32_t log2_l = 0;     // SRC_CELLS: the cell size; vector j is stride j
    uint32_t n_lane = 0;     // n_vec << (k - 1) butterflies, or n_vec points for k = 0 (a copy)
};
constexpr int64_t SRC_INFINITY = -1;
// SRC_WIRE: the index of the wire point; SRC_SETUP: the index of the monomial point of position e of (s_{N-2}, .., s_0, inf x (N + 1)),
// k = log2(2 N); SRC_REC: the record.  SRC_INFINITY: the identity
// SRC_CELLS (the cell proofs' setup, zkp_cells_plan.hpp): the index of the monomial point of position pe of vector i < l,
// (s_{N-l-1-i}, s_{N-2l-1-i}, .., k - 1 points with the index stepping down by l, then k + 1 identities), k1 = log2(2 k) >= 1
ZKP_FK20_HD int64_t cells_setup_source(uint32_t log2_l, uint32_t k1, uint32_t i, uint32_t pe) {
    const uint32_t k = 1u << (k1 - 1);
    return pe + 2 <= k ? (int64_t)(((uint64_t)(k - 1 - pe) << log2_l) - 1 - i) : SRC_INFINITY;
}
ZKP_FK20_HD int64_t first_source(const First& a, uint32_t j, uint32_t e) {
    const uint32_t k = a.at.k, pe = a.perm ? bitrev(e, k) : e;
    if (a.mode == SRC_REC) return a.src_len && pe >= a.src_len ? SRC_INFINITY : (int64_t)((j << a.at.vs_log2) + a.src_off + pe);
    if (a.mode == SRC_WIRE) return (int64_t)(((uint64_t)j << k) + pe);
    if (a.mode == SRC_CELLS) return cells_setup_source(a.log2_l, k, j, pe);
    const uint32_t n = 1u << (k - 1);                 // SRC_SETUP: k >= 1
    return pe + 2 <= n ? (int64_t)(n - 2 - pe) : SRC_INFINITY;
}

// ---- the last kernel: record -> wire ----------------------------------------------------------------------------------------------------
struct Out {
    Span at;
    uint32_t perm = 0;       // position e goes to slot bitrev(e)
    uint32_t scale = 0;      // multiply by the split scalar of the launch (the inverse's N^-1)
    uint32_t n_pt = 0;       // n_vec << k
};
ZKP_FK20_HD void out_lane(const Out& a, uint32_t t, uint32_t* rec, uint64_t* slot) {
    const uint32_t k = a.at.k, j = t >> k, e = t & low_mask(k);
    *rec = span_record(a.at, j, e);
    *slot = ((uint64_t)j << k) + (a.perm ? bitrev(e, k) : e);
}

// ---- FK20: entry i of c = (f_{N-1}, 0 x (N + 1), f_1, .., f_{N-2}), k = log2 N: the coefficient's index, or -1 for zero ------------------
ZKP_FK20_HD int64_t coeff_source(uint32_t i, uint32_t k) {
    const uint32_t n = 1u << k;
    if (i == 0) return (int64_t)n - 1;
    return i >= n + 2 ? (int64_t)(i - n - 1) : -1;
}

// ---- the split of a scalar at z^2: s = a + b z^2 with a = s mod z^2, b = floor(s / z^2).  z^2 < 2^128 and s < r = z^4 - z^2 + 1 < z^4 give
// a, b < z^2 < 2^128.  Restoring division, one bit of s per step; s and the results are little-endian 32-bit words.
constexpr uint32_t Z2[4] = {0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u};
ZKP_FK20_HD void split_z2(const uint32_t* s, uint32_t* a, uint32_t* b) {
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, q[8];
    ZKP_FK20_UNROLL
    for (int w = 7; w >= 0; w--) {     // every array index is a constant once this loop is unrolled
        const uint32_t word = s[w];
        uint32_t qw = 0;
        ZKP_FK20_NOUNROLL
        for (int bit = 31; bit >= 0; bit--) {
            r4 = (r4 << 1) | (r3 >> 31);
            r3 = (r3 << 1) | (r2 >> 31);
            r2 = (r2 << 1) | (r1 >> 31);
            r1 = (r1 << 1) | (r0 >> 31);
            r0 = (r0 << 1) | ((word >> bit) & 1u);
            int64_t bw = (int64_t)r0 - Z2[0];
            const uint32_t t0 = (uint32_t)bw;
            bw = (bw >> 32) + (int64_t)r1 - Z2[1];
            const uint32_t t1 = (uint32_t)bw;
            bw = (bw >> 32) + (int64_t)r2 - Z2[2];
            const uint32_t t2 = (uint32_t)bw;
            bw = (bw >> 32) + (int64_t)r3 - Z2[3];
            const uint32_t t3 = (uint32_t)bw;
            bw = (bw >> 32) + (int64_t)r4;
            const uint32_t t4 = (uint32_t)bw;
            const bool ge = (bw >> 32) == 0;     // no borrow: the remainder reached z^2
            r0 = ge ? t0 : r0;
            r1 = ge ? t1 : r1;
            r2 = ge ? t2 : r2;
            r3 = ge ? t3 : r3;
            r4 = ge ? t4 : r4;
            qw = (qw << 1) | (ge ? 1u : 0u);
        }
        q[w] = qw;
    }
    a[0] = r0;
    a[1] = r1;
    a[2] = r2;
    a[3] = r3;
    ZKP_FK20_UNROLL
    for (int i = 0; i < 4; i++) b[i] = q[i];
}

}  // namespace fk20
}  // namespace zkp
