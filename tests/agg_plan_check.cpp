// The planning header of the G1 segment sums and FastAggregateVerify (zkp_bls_agg_plan.hpp) walked at the limits of the C ABI and on both
// sides of every power of msm::RUN, where the run-wise sum gains a level; built with g++ -fsanitize=address,undefined and run as a child
// process by tests/test_agg_cpu.py.
#include <cassert>
#include <cstdio>
#include <vector>
#include "zkp_bls_agg_plan.hpp"
using namespace zkp;
using namespace zkp::agg;

// the launches of the driver's loop (sums_into, zkp_bls_agg.hip): (entries read, buffer written)
static int drive(size_t n_idx, const Plan& p) {
    uint32_t n = (uint32_t)n_idx;
    int lv = 0;
    for (; n; lv++) {
        assert(lv < p.levels && p.level_in[lv] == n);
        assert(2 * msm::runs_of(n) <= p.part_cap[lv & 1]);               // what the level writes fits its buffer
        if (lv) assert(n <= p.part_cap[(lv - 1) & 1]);                   // what it reads is what the level before wrote
        if (n <= msm::RUN) { lv++; break; }
        n = 2 * msm::runs_of(n);
    }
    return lv;
}

int main() {
    static_assert(MAX_IDX == ((size_t)1 << 26) && MAX_TABLE == ((size_t)1 << 24) && MAX_SEG == ((size_t)1 << 24), "the header's limits");
    static_assert(((uint64_t)1 << SEARCH_STEPS) > MAX_SEG + 1, "the bounded search reaches every segment");
    static_assert(POINT_REC == 128 && JAC_REC == 192, "the header's workspace figures");
    static_assert(!args_bad(0, 0, 0) && !args_bad(MAX_TABLE, MAX_IDX, MAX_SEG) && args_bad(MAX_TABLE + 1, 0, 0) && args_bad(1, MAX_IDX + 1, 1) &&
                      args_bad(1, 1, MAX_SEG + 1) && args_bad(0, 1, 1) && !args_bad(0, 0, 5) && !args_bad(1, 1, 0),
                  "args_bad");
    std::vector<size_t> sizes = {0, 1, 2, 31, 63, 64, 65, MAX_IDX - 1, MAX_IDX};
    for (size_t pw = msm::RUN; pw <= MAX_IDX; pw *= msm::RUN)
        for (size_t d = 0; d < 3; d++) sizes.push_back(pw - 1 + d);      // 32^k - 1, 32^k, 32^k + 1
    for (size_t t = msm::RUN; t <= MAX_IDX; t *= msm::RUN / 2)           // 32 * 16^k: where the sum gains a level (two partials per run of 32)
        for (size_t d = 0; d < 3; d++) sizes.push_back(t - 1 + d);
    for (size_t n : sizes) {
        if (n > MAX_IDX) continue;
        const Plan p = make_plan(n);
        assert(p.levels <= msm::MAX_LEVELS && drive(n, p) == p.levels);
        // a level halves sixteen-fold: n <= 32 one level, <= 512 two, <= 8192 three
        int want = 0;
        for (size_t v = n; v; v = v <= msm::RUN ? 0 : 2 * msm::runs_of((uint32_t)v)) want++;
        assert(p.levels == want);
        if (n) assert(p.level_in[p.levels - 1] <= msm::RUN && (p.levels == 1 || p.level_in[p.levels - 2] > msm::RUN));
    }
    assert(make_plan(32).levels == 1 && make_plan(33).levels == 2 && make_plan(512).levels == 2 && make_plan(513).levels == 3);
    assert(make_plan(8192).levels == 3 && make_plan(8193).levels == 4 && make_plan(MAX_IDX).levels == 7);
    const size_t tables[] = {0, 1, 37, MAX_TABLE}, segs[] = {0, 1, 63, 64, 65, MAX_SEG};
    for (size_t n_table : tables)
        for (size_t n_idx : sizes)
            for (size_t n_seg : segs)
                for (int verify = 0; verify < 2; verify++) {
                    if (n_idx > MAX_IDX || args_bad(n_table, n_idx, n_seg)) continue;
                    const Plan p = make_plan(n_idx);
                    const Layout L = layout(n_table, n_idx, n_seg, verify != 0);
                    const size_t o[] = {L.pts, L.keys, L.vals, L.part_k[0], L.part_j[0], L.part_k[1], L.part_j[1], L.word, L.sums, L.apk, L.apk_inf, L.st, L.total};
                    for (int i = 0; i + 1 < 13; i++) assert(o[i] % 256 == 0 && o[i] <= o[i + 1]);
                    assert(L.keys - L.pts >= n_table * 128 && L.vals - L.keys >= n_idx * 4 && L.part_k[0] - L.vals >= n_idx * 4);
                    for (int i = 0; i < 2; i++) {
                        assert(L.part_j[i] - L.part_k[i] >= (size_t)p.part_cap[i] * 4);
                        assert((i ? L.word : L.part_k[1]) - L.part_j[i] >= (size_t)p.part_cap[i] * 192);
                    }
                    assert(L.sums == L.word + 256 && L.fill == 256 + n_seg * 192 && L.fill % 16 == 0 && L.word + L.fill <= L.apk);
                    if (verify) assert(L.apk_inf - L.apk >= 96 * n_seg && L.st - L.apk_inf >= n_seg && L.total - L.st >= n_seg);
                    else assert(L.total == L.apk);
                    assert(L.total < ((size_t)1 << 36));
                }
    // the host flavour's two refusals
    const uint64_t good[] = {0, 0, 3, 3, 5}, dec[] = {0, 4, 3, 5, 5}, first[] = {1, 1, 3, 3, 5}, beyond[] = {0, 0, 3, 3, 6}, below[] = {0, 0, 3, 3, 4};
    assert(!offsets_malformed(good, 4, 5) && offsets_malformed(dec, 4, 5) && offsets_malformed(first, 4, 5) && offsets_malformed(beyond, 4, 5) &&
           offsets_malformed(below, 4, 5));
    const uint64_t none[] = {0};
    assert(!offsets_malformed(none, 0, 0) && offsets_malformed(none, 0, 1));
    const uint32_t rows[] = {0, 36, 36u | SIGN, 5};
    assert(!rows_out_of_range(rows, 4, 37) && rows_out_of_range(rows, 4, 36) && !rows_out_of_range(rows, 0, 0));
    const uint32_t top[] = {ROW_MASK}, topneg[] = {0xffffffffu};
    assert(rows_out_of_range(top, 1, MAX_TABLE) && rows_out_of_range(topneg, 1, MAX_TABLE));
    std::puts("ok");
    return 0;
}
