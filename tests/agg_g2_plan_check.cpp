// The planning header of the G2 segment sums, the min-sig FastAggregateVerify and AggregateVerify (zkp_bls_agg_g2_plan.hpp) walked at the
// limits of the C ABI, at 0 and 1, and on both sides of every power of msm::RUN, where the run-wise sum gains a level; built with
// g++ -fsanitize=address,undefined and run as a child process by tests/test_agg_g2_cpu.py.
#include <cassert>
#include <cstdio>
#include <vector>
#include "zkp_bls_agg_g2_plan.hpp"
using namespace zkp;
using namespace zkp::agg2;

int main() {
    static_assert(MAX_IDX == ((size_t)1 << 26) && MAX_TABLE == ((size_t)1 << 24) && MAX_SEG == ((size_t)1 << 24) && MAX_MSG == ((size_t)1 << 24),
                  "the header's limits");
    static_assert(((uint64_t)1 << agg::SEARCH_STEPS) > MAX_SEG + 1, "the bounded search reaches every segment");
    static_assert(POINT_REC == 256 && JAC_REC == 384 && ENTRY_BYTES == 8 && PART_BYTES == 388 && SEG_BYTES == 384 && APK_BYTES == 194 && MSG_BYTES == 209,
                  "the header's workspace figures");
    static_assert(MAX_TABLE * POINT_REC == ((size_t)4 << 30), "4 GB of Montgomery records at the largest table");
    static_assert(!args_bad(0, 0, 0) && !args_bad(MAX_TABLE, MAX_IDX, MAX_SEG) && args_bad(MAX_TABLE + 1, 0, 0) && args_bad(1, MAX_IDX + 1, 1) &&
                      args_bad(1, 1, MAX_SEG + 1) && args_bad(0, 1, 1) && !args_bad(0, 0, 5) && !args_bad(1, 1, 0),
                  "args_bad");
    static_assert(!verify_args_bad(0, 0) && !verify_args_bad(1, 1) && !verify_args_bad(MAX_MSG, MAX_SEG) && verify_args_bad(MAX_MSG + 1, 1) &&
                      verify_args_bad(1, MAX_SEG + 1) && !verify_args_bad(5, 0) && !verify_args_bad(0, 5),
                  "verify_args_bad");
    static_assert(4 * MAX_TABLE <= 0xffffffffu, "the field elements of the largest table are counted in 32 bits");
    std::vector<size_t> sizes = {0, 1, 2, 31, 63, 64, 65, MAX_IDX - 1, MAX_IDX};
    for (size_t pw = msm::RUN; pw <= MAX_IDX; pw *= msm::RUN)
        for (size_t d = 0; d < 3; d++) sizes.push_back(pw - 1 + d);
    for (size_t t = msm::RUN; t <= MAX_IDX; t *= msm::RUN / 2)
        for (size_t d = 0; d < 3; d++) sizes.push_back(t - 1 + d);
    const size_t tables[] = {0, 1, 37, MAX_TABLE}, segs[] = {0, 1, 63, 64, 65, MAX_SEG};
    for (size_t n_table : tables)
        for (size_t n_idx : sizes)
            for (size_t n_seg : segs)
                for (int verify = 0; verify < 2; verify++) {
                    if (n_idx > MAX_IDX || args_bad(n_table, n_idx, n_seg)) continue;
                    // the level capacities are msm::level_chain's: what a level writes fits its buffer, what it reads is what the level before wrote
                    const agg::Plan p = agg::make_plan(n_idx);
                    uint32_t in[msm::MAX_LEVELS] = {}, cap[2] = {};
                    const int levels = n_idx ? msm::level_chain((uint32_t)n_idx, in, cap) : 0;
                    assert(levels == p.levels && cap[0] == p.part_cap[0] && cap[1] == p.part_cap[1] && levels <= msm::MAX_LEVELS);
                    for (int lv = 0; lv < levels; lv++) {
                        assert(in[lv] == p.level_in[lv] && 2 * msm::runs_of(in[lv]) <= p.part_cap[lv & 1]);
                        if (lv) assert(in[lv] <= p.part_cap[(lv - 1) & 1]);
                    }
                    const Layout L = layout(n_table, n_idx, n_seg, verify != 0);
                    const size_t o[] = {L.pts, L.keys, L.vals, L.part_k[0], L.part_j[0], L.part_k[1], L.part_j[1], L.word, L.sums, L.apk, L.apk_inf, L.st, L.total};
                    for (int i = 0; i + 1 < 13; i++) assert(o[i] % 256 == 0 && o[i] <= o[i + 1]);
                    assert(L.keys - L.pts >= n_table * 256 && L.vals - L.keys >= n_idx * 4 && L.part_k[0] - L.vals >= n_idx * 4);
                    for (int i = 0; i < 2; i++) {
                        assert(L.part_j[i] - L.part_k[i] >= (size_t)p.part_cap[i] * 4);
                        assert((i ? L.word : L.part_k[1]) - L.part_j[i] >= (size_t)p.part_cap[i] * 384);
                    }
                    assert(L.sums == L.word + 256 && L.fill == 256 + n_seg * 384 && L.fill % 16 == 0 && L.word + L.fill <= L.apk);
                    if (verify) assert(L.apk_inf - L.apk >= 192 * n_seg && L.st - L.apk_inf >= n_seg && L.total - L.st >= n_seg);
                    else assert(L.total == L.apk);
                    assert(L.total < ((size_t)1 << 37));
                }
    assert(layout(0, 0, 0, false).total == 256 && layout(1, 1, 1, false).total == 3 * 256 + (256 + 768) + 256 + 512);
    const size_t msgs[] = {0, 1, 2, 255, 256, 257, ((size_t)1 << 17) + 6, MAX_MSG}, sigs[] = {0, 1, 63, 64, 65, MAX_SEG};
    for (size_t n_msg : msgs)
        for (size_t n : sigs) {
            if (verify_args_bad(n_msg, n)) continue;
            const Expand E = expand_layout(n_msg, n);
            const size_t o[] = {E.word, E.st, E.sig, E.inf_sig, E.rand, E.total};
            for (int i = 0; i + 1 < 6; i++) assert(o[i] % 256 == 0 && o[i] <= o[i + 1]);
            assert(E.word == 0 && E.st == 256 && E.sig - E.st >= n && E.inf_sig - E.sig >= n_msg * 192 && E.rand - E.inf_sig >= n_msg &&
                   E.total - E.rand >= n_msg * 16);
            assert(E.total < ((size_t)1 << 33));
        }
    assert(expand_layout(0, 0).total == 256 && expand_layout(1, 1).total == 256 * 5);
    std::puts("ok");
    return 0;
}
