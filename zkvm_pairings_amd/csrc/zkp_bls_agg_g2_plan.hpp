// zkp_bls_agg_g2_plan.hpp -- limits and workspace layouts of the G2 segment sums, of the min-sig FastAggregateVerify and of AggregateVerify
// (zkp_bls_agg_g2.hip).  The entries, the offsets, the search and the levels of the run-wise segmented sum are those of the G1 sums
// (zkp_bls_agg_plan.hpp, msm::level_chain); what differs is the size of a point.  Both layouts live in the context's aggregation
// workspace (ctxop::grow_agg), one call at a time.  Plain C++: a host compiler takes it (tests/agg_g2_plan_check.cpp walks it under
// sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zkp_bls_agg_plan.hpp"
#include "zkp_bls_plan.hpp"

namespace zkp {
namespace agg2 {

constexpr size_t MAX_TABLE = agg::MAX_TABLE;         // rows of the table: 2^24, 4 GB of Montgomery records
constexpr size_t MAX_IDX = agg::MAX_IDX;
constexpr size_t MAX_SEG = agg::MAX_SEG;
constexpr size_t MAX_MSG = bls::MAX_VERIFY_N;        // AggregateVerify: messages of one call (the limit of zkp_bls_verify_batch)
constexpr size_t POINT_REC = 4 * msm::REC_BYTES;     // a table point: x.c0, x.c1, y.c0, y.c1
constexpr size_t JAC_REC = 6 * msm::REC_BYTES;       // a Jacobian sum or partial: x.c0, x.c1, y.c0, y.c1, z.c0, z.c1
constexpr size_t ENTRY_BYTES = 8;                    // a key and a value per entry
constexpr size_t PART_BYTES = 4 + JAC_REC;           // a partial sum and its key
constexpr size_t SEG_BYTES = JAC_REC;                // per segment; the verifier adds APK_BYTES
constexpr size_t APK_BYTES = 192 + 2;                // the verifier's aggregate key in wire format, its infinity byte, its status
constexpr size_t MSG_BYTES = 192 + 1 + 16;           // AggregateVerify per message: the expanded signature, its infinity byte, its rand row

// the ABI's argument check on the three counts of a sum: the G1 rule
constexpr bool args_bad(size_t n_table, size_t n_idx, size_t n_seg) { return agg::args_bad(n_table, n_idx, n_seg); }
// ... and on the two counts of AggregateVerify (messages without a signature are malformed input, not a bad argument)
constexpr bool verify_args_bad(size_t n_msg, size_t n) { return n_msg > MAX_MSG || n > MAX_SEG; }

struct Layout {
    size_t pts, keys, vals, part_k[2], part_j[2], word, sums, apk, apk_inf, st, total;
    size_t fill;                                     // bytes of the fill from `word`: the word's 256 and the sums
};
inline Layout layout(size_t n_table, size_t n_idx, size_t n_seg, bool verify) {
    Layout L;
    const agg::Plan p = agg::make_plan(n_idx);
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
    L.apk = take(verify ? n_seg * 192 : 0);
    L.apk_inf = take(verify ? n_seg : 0);
    L.st = take(verify ? n_seg : 0);
    L.total = at;
    return L;
}

// AggregateVerify: the call's word, a status byte per signature (k_agg_check zeroes them, k_agg_fold reads them) and the three expanded
// arrays that zkp_bls_verify_batch's driver reads in place of the caller's
struct Expand {
    size_t word, st, sig, inf_sig, rand, total;
};
inline Expand expand_layout(size_t n_msg, size_t n) {
    Expand L;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += msm::align256(bytes); return o; };
    L.word = take(256);
    L.st = take(n);
    L.sig = take(n_msg * 192);
    L.inf_sig = take(n_msg);
    L.rand = take(n_msg * 16);
    L.total = at;
    return L;
}

}  // namespace agg2
}  // namespace zkp
