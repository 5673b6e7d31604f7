// zkp_msm_plan.hpp -- the host side's PURE arithmetic of the bucket multi-scalar multiplication (zkp_g1/g2_msm_batch): window
// width, window count, how many segments one pass takes, the sizes of every workspace region and every launch count.  No HIP type,
// no allocation, no I/O: included by zkp_msm.hip (the product) and compiled with gcc -fsanitize=address,undefined by
// tests/test_msm_cpu.py, which walks it over the sizes the C ABI admits and asserts that every per-launch count fits 32 bits.
//
// Terms: an MSM call is n_msm independent sums ("segments") of m terms each.  A scalar (256 bits) is cut into W = 256/c + 1
// signed digits of c bits, d in [-2^(c-1) + 1, 2^(c-1)]; digit (segment s, window w, |d|) falls into bucket
// (s * W + w) * 2^(c-1) + |d| - 1.  One sort key per non-zero digit.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkp {
namespace msm {

constexpr size_t MAX_TERMS = (size_t)1 << 24;        // ABI maximum of m * n_msm
constexpr uint32_t RUN = 32;                         // sorted entries one lane (G1) / lane pair (G2) accumulates
constexpr uint32_t KEY_NONE = 0x7fffffffu;           // key of a dropped digit (zero digit, point at infinity): sorts last
constexpr uint32_t KEY_FLAG = 0x80000000u;           // partial sums: "holds a real contribution" (masked off before comparing)
constexpr size_t KEYS_PER_PASS = (size_t)1 << 26;    // a pass takes whole segments up to this many keys (or one segment)
constexpr uint32_t MAX_BUCKETS = 1u << 24;           // per pass, or one segment's (at most 17 * 2^15): 3.2 GB of G1 buckets
constexpr uint32_t REDUCE_LANES = 1u << 15;          // the bucket reduction aims at this many lanes (or lane pairs) per pass
constexpr int MAX_LEVELS = 16;
constexpr uint32_t REC_BYTES = 64;                   // one Fp in the 28-bit core: 14 limbs in four int4

// the ABI's argument check: m >= 1 when there is any segment, m * n_msm <= 2^24
constexpr bool msm_args_bad(size_t m, size_t n_msm) { return n_msm && (m == 0 || m > MAX_TERMS || n_msm > MAX_TERMS / m); }

inline uint32_t windows_for(uint32_t c) { return 256 / c + 1; }

// window width: the c of 2..16 with the fewest group operations per segment, W * (m + 3 * 2^(c-1)) - one mixed addition per
// term and window, about three additions per bucket in the reduction (two running sums, the fix-up and the chunk scaling)
inline uint32_t choose_c(size_t m) {
    uint32_t best = 2;
    double best_cost = 0;
    for (uint32_t c = 2; c <= 16; c++) {
        const double cost = (double)windows_for(c) * ((double)m + 3.0 * (double)(1u << (c - 1)));
        if (c == 2 || cost < best_cost) { best = c; best_cost = cost; }
    }
    return best;
}

struct Plan {
    uint32_t c = 0, windows = 0, nb = 0;       // window bits, windows per scalar, buckets per window (2^(c-1))
    uint32_t segs = 0, passes = 0;             // segments per pass, passes
    uint32_t terms = 0;                        // terms per pass (segs * m)
    uint32_t pts = 0;                          // points converted per pass (m when shared, else terms)
    uint32_t keys = 0;                         // sort keys per pass (terms * windows)
    uint32_t key_bits = 0;                     // radix sort end bit: bucket ids < 2^key_bits, KEY_NONE's low bits above all of them
    uint32_t buckets = 0;                      // per pass: segs * windows * nb
    uint32_t split = 0, chunk = 0;             // bucket reduction: lanes per window, buckets per lane (split * chunk = nb)
    uint32_t sums = 0;                         // window sums per pass (segs * windows); the reduction writes sums * split chunk sums
    int levels = 0;                            // accumulation launches (level 0 from the sorted digits, then fix-ups)
    uint32_t level_in[MAX_LEVELS] = {};        // entries each accumulation level reads
    int wlevels = 0;                           // fix-up launches joining the chunk sums into window sums
    uint32_t wlevel_in[MAX_LEVELS] = {};
    uint32_t part_cap[2] = {};                 // entries of the partial-sum ping-pong buffers (level l writes buffer l & 1)
};

inline uint32_t runs_of(uint32_t n) { return (n + RUN - 1) / RUN; }

// levels of the run-wise segmented sum of n sorted entries: each level leaves two partial sums per run (also the last, which has
// ONE run); level l writes them to buffer l & 1
inline int level_chain(uint32_t n, uint32_t* in, uint32_t* cap) {
    for (int lv = 0;; lv++) {
        in[lv] = n;
        const uint32_t o = 2 * runs_of(n);
        if (o > cap[lv & 1]) cap[lv & 1] = o;
        if (n <= RUN) return lv + 1;
        n = o;
    }
}

inline uint32_t bits_for(uint32_t v) { uint32_t b = 1; while (b < 31 && (1u << b) <= v) b++; return b; }

// ok == false: the sizes are outside the ABI (msm_args_bad) - never the case for admitted arguments
inline bool make_plan(size_t m, size_t n_msm, bool shared, Plan* p) {
    *p = Plan();
    if (msm_args_bad(m, n_msm) || n_msm == 0) return false;
    p->c = choose_c(m);
    p->windows = windows_for(p->c);
    p->nb = 1u << (p->c - 1);
    const size_t per_seg_keys = m * p->windows, per_seg_buckets = (size_t)p->windows * p->nb;
    size_t segs = per_seg_keys >= KEYS_PER_PASS ? 1 : KEYS_PER_PASS / per_seg_keys;
    if (segs * per_seg_buckets > MAX_BUCKETS) segs = MAX_BUCKETS / per_seg_buckets;
    if (segs > n_msm) segs = n_msm;
    if (segs < 1) segs = 1;
    p->segs = (uint32_t)segs;
    p->passes = (uint32_t)((n_msm + segs - 1) / segs);
    p->terms = (uint32_t)(segs * m);
    p->pts = shared ? (uint32_t)m : p->terms;
    p->keys = (uint32_t)(segs * per_seg_keys);
    p->buckets = (uint32_t)(segs * per_seg_buckets);
    p->key_bits = bits_for(p->buckets);
    p->sums = (uint32_t)(segs * p->windows);
    uint32_t split = 1;
    while (split < p->nb && (size_t)p->sums * split * 2 <= REDUCE_LANES) split *= 2;
    p->split = split;
    p->chunk = p->nb / split;
    p->levels = level_chain(p->keys, p->level_in, p->part_cap);
    p->wlevels = level_chain(p->sums * p->split, p->wlevel_in, p->part_cap);
    return true;
}

// workspace layout (bytes; every region 256-byte aligned).  np: Fp records per point (2 for G1, 4 for G2), jr: bytes of one
// Jacobian record (3 * np / 2 Fp records).  sort_temp: what the radix sort asks for at p.keys entries.
struct Layout {
    size_t pts, keys_in, vals_in, keys_out, vals_out, sort_temp, buckets, part_k[2], part_j[2], chunk_k, chunk_j, wsums, total;
};
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline Layout make_layout(const Plan& p, uint32_t np, size_t sort_temp) {
    Layout L;
    const size_t jr = (size_t)3 * (np / 2) * REC_BYTES;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    L.pts = take((size_t)p.pts * np * REC_BYTES);
    L.keys_in = take((size_t)p.keys * 4);
    L.vals_in = take((size_t)p.keys * 4);
    L.keys_out = take((size_t)p.keys * 4);
    L.vals_out = take((size_t)p.keys * 4);
    L.sort_temp = take(sort_temp);
    L.buckets = take((size_t)p.buckets * jr);
    for (int i = 0; i < 2; i++) {
        L.part_k[i] = take((size_t)p.part_cap[i] * 4);
        L.part_j[i] = take((size_t)p.part_cap[i] * jr);
    }
    L.chunk_k = take((size_t)p.sums * p.split * 4);
    L.chunk_j = take((size_t)p.sums * p.split * jr);
    L.wsums = take((size_t)p.sums * jr);
    L.total = o;
    return L;
}

}  // namespace msm
}  // namespace zkp
