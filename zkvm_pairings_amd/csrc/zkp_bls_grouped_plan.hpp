// zkp_bls_grouped_plan.hpp -- limits and workspace layout of the scaled G1 segment sums and of the BLS verifier grouped by message
// (zkp_bls_grouped.hip): the levels of the run-wise segmented sum come from msm::level_chain, as the bucket MSM's and zkp_bls_agg_plan.hpp's
// do.  Plain C++: a host compiler takes it (tests/grp_plan_check.cpp walks it under sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zkp_msm_plan.hpp"

namespace zkp {
namespace grp {

constexpr size_t MAX_N = (size_t)1 << 24;            // points / signatures of one call: also bls::MAX_VERIFY_N and the MSM's term limit
constexpr size_t MAX_SEG = (size_t)1 << 24;          // segments / distinct messages of one call
constexpr int SEARCH_STEPS = 25;                     // the bounded search of a signature's group: 2^25 > MAX_SEG + 1 offsets
constexpr size_t JAC_REC = 3 * msm::REC_BYTES;       // a scaled key and a Jacobian sum
constexpr size_t ML_RECORDS = 3;                     // Miller values of the m message pairs and of (-g1, S), then Gt

// the ABI's argument check on the two counts (pointers are the entry points' business)
constexpr bool args_bad(size_t n, size_t n_seg) { return n > MAX_N || n_seg > MAX_SEG; }

// host offsets: non-decreasing from 0 to n
inline bool offsets_malformed(const uint64_t* seg_off, size_t n_seg, size_t n) {
    if (seg_off[0] != 0 || seg_off[n_seg] != n) return true;
    for (size_t j = 0; j < n_seg; j++)
        if (seg_off[j + 1] < seg_off[j]) return true;
    return false;
}

struct Plan {
    int levels = 0;                                  // accumulation launches: every level reads Jacobian records (the scaled keys first)
    uint32_t level_in[msm::MAX_LEVELS] = {};         // records each level reads
    uint32_t part_cap[2] = {};                       // records of the two partial-sum buffers (level l writes buffer l & 1)
};
inline Plan make_plan(size_t n) {
    Plan p;
    if (n) p.levels = msm::level_chain((uint32_t)n, p.level_in, p.part_cap);
    return p;
}

// workspace (bytes; every region 256-byte aligned): one word (the call is malformed) in front of the sums so that one fill zeroes both,
// 192 B per segment, 4 + 192 B per point (key and scaled key), the two partial levels (4 + 192 B per partial); for the verifier 32 + 2 B
// per signature (the MSM's scalar, two status bytes), 96 + 2 + 192 + 1 B per message (A_g, its infinity byte and status, H_g, its infinity
// byte), the flag words, -g1, S and three Fp12 records
struct Layout {
    size_t word, sums, keys, jrec, part_k[2], part_j[2];
    size_t flag, sc, st, apk, apk_inf, apk_st, hq, hinf, neg_g1, neg_g1_inf, s, s_inf, ml, total;
    size_t fill;                                     // bytes of the fill from `word`: the word's 256 and the sums
};
inline Layout layout(size_t n, size_t n_seg, bool verify) {
    Layout L;
    const Plan p = make_plan(n);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += msm::align256(bytes); return o; };
    L.word = take(256);
    L.sums = take(n_seg * JAC_REC);
    L.fill = 256 + n_seg * JAC_REC;
    L.keys = take(n * 4);
    L.jrec = take(n * JAC_REC);
    for (int i = 0; i < 2; i++) {
        L.part_k[i] = take((size_t)p.part_cap[i] * 4);
        L.part_j[i] = take((size_t)p.part_cap[i] * JAC_REC);
    }
    L.flag = take(verify ? 4 * sizeof(int32_t) : 0);
    L.sc = take(verify ? n * 32 : 0);
    L.st = take(verify ? 2 * n : 0);
    L.apk = take(verify ? n_seg * 96 : 0);
    L.apk_inf = take(verify ? n_seg : 0);
    L.apk_st = take(verify ? n_seg : 0);
    L.hq = take(verify ? n_seg * 192 : 0);
    L.hinf = take(verify ? n_seg : 0);
    L.neg_g1 = take(verify ? 96 : 0);
    L.neg_g1_inf = take(verify ? 1 : 0);
    L.s = take(verify ? 192 : 0);
    L.s_inf = take(verify ? 1 : 0);
    L.ml = take(verify ? ML_RECORDS * 576 : 0);
    L.total = at;
    return L;
}

}  // namespace grp
}  // namespace zkp
