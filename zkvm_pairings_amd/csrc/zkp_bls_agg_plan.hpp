// zkp_bls_agg_plan.hpp -- limits and workspace layout of the G1 segment sums and of FastAggregateVerify (zkp_bls_agg.hip): the levels of
// the run-wise segmented sum come from msm::level_chain, as the bucket MSM's do.  Plain C++: a host compiler takes it
// (tests/agg_plan_check.cpp walks it under sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zkp_msm_plan.hpp"

namespace zkp {
namespace agg {

constexpr size_t MAX_TABLE = (size_t)1 << 24;        // rows of the key table: 2 GB of Montgomery records
constexpr size_t MAX_IDX = msm::KEYS_PER_PASS;       // entries of one call: every count the accumulation kernel sees stays in 32 bits
constexpr size_t MAX_SEG = (size_t)1 << 24;          // segments of one call; for the verifier also bls::MAX_VERIFY_N
constexpr uint32_t SIGN = 0x80000000u;               // bit 31 of an entry: subtract the row
constexpr uint32_t ROW_MASK = 0x7fffffffu;
constexpr int SEARCH_STEPS = 25;                     // the bounded search of an entry's segment: 2^25 > MAX_SEG + 1 offsets
constexpr size_t POINT_REC = 2 * msm::REC_BYTES;     // a table point as two Montgomery records
constexpr size_t JAC_REC = 3 * msm::REC_BYTES;       // a Jacobian sum

// the ABI's argument check on the three counts (pointers are the entry points' business)
constexpr bool args_bad(size_t n_table, size_t n_idx, size_t n_seg) {
    return n_table > MAX_TABLE || n_idx > MAX_IDX || n_seg > MAX_SEG || (n_idx && !n_table);
}

// host offsets: non-decreasing from 0 to n_idx
inline bool offsets_malformed(const uint64_t* seg_off, size_t n_seg, size_t n_idx) {
    if (seg_off[0] != 0 || seg_off[n_seg] != n_idx) return true;
    for (size_t j = 0; j < n_seg; j++)
        if (seg_off[j + 1] < seg_off[j]) return true;
    return false;
}
// host entries: every row below n_table
inline bool rows_out_of_range(const uint32_t* idx, size_t n_idx, size_t n_table) {
    for (size_t e = 0; e < n_idx; e++)
        if ((idx[e] & ROW_MASK) >= n_table) return true;
    return false;
}

struct Plan {
    int levels = 0;                                  // accumulation launches: level 0 from the entries, then the partial sums
    uint32_t level_in[msm::MAX_LEVELS] = {};         // entries each level reads
    uint32_t part_cap[2] = {};                       // entries of the two partial-sum buffers (level l writes buffer l & 1)
};
inline Plan make_plan(size_t n_idx) {
    Plan p;
    if (n_idx) p.levels = msm::level_chain((uint32_t)n_idx, p.level_in, p.part_cap);
    return p;
}

// workspace (bytes; every region 256-byte aligned): 128 B per table point, 8 B per entry, the two partial levels (4 + 192 B per partial), one
// word (the call is malformed) in front of the sums so that one fill zeroes both, 192 B per segment; for the verifier 96 + 2 B per committee
struct Layout {
    size_t pts, keys, vals, part_k[2], part_j[2], word, sums, apk, apk_inf, st, total;
    size_t fill;                                     // bytes of the fill from `word`: the word's 256 and the sums
};
inline Layout layout(size_t n_table, size_t n_idx, size_t n_seg, bool verify) {
    Layout L;
    const Plan p = make_plan(n_idx);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += msm::align256(bytes); return o; };
    L.pts = take(n_table * POINT_REC);
    L.keys = take(n_idx * 4);
    L.vals = take(n_idx * 4);
    for (int i = 0; i < 2; i++) {
        L.part_k[i] = take((size_t)p.part_cap[i] * 4);
        L.part_j[i] = take((size_t)p.part_cap[i] * JAC_REC);
    }
    L.word = take(256);
    L.sums = take(n_seg * JAC_REC);
    L.fill = 256 + n_seg * JAC_REC;
    L.apk = take(verify ? n_seg * 96 : 0);
    L.apk_inf = take(verify ? n_seg : 0);
    L.st = take(verify ? n_seg : 0);
    L.total = at;
    return L;
}

}  // namespace agg
}  // namespace zkp
