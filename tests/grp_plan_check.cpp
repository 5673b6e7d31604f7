// The planning header of the scaled segment sums and the grouped verifiers (zkp_bls_grouped_plan.hpp) walked at the limits of the C ABI
// and on both sides of every power of msm::RUN, where the run-wise sum gains a level; built with g++ -fsanitize=address,undefined and run
// as a child process by tests/test_grp_cpu.py.
#include <cassert>
#include <cstdio>
#include <vector>
#include "zkp_bls_grouped_plan.hpp"
using namespace zkp;
using namespace zkp::grp;

// the launches of the driver's loop (sums_into, zkp_bls_grouped.hip): (records read, buffer written)
static int drive(size_t n_pts, const Plan& p) {
    uint32_t n = (uint32_t)n_pts;
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
    static_assert(MAX_N == ((size_t)1 << 24) && MAX_SEG == ((size_t)1 << 24), "the header's limits");
    static_assert(MAX_N <= msm::MAX_TERMS && MAX_N <= msm::KEYS_PER_PASS, "the G2 MSM takes the call's signatures; every count stays in 32 bits");
    static_assert(((uint64_t)1 << SEARCH_STEPS) > MAX_SEG + 1, "the bounded search reaches every group");
    static_assert(JAC_REC == 192 && ML_RECORDS == 3, "the header's workspace figures");
    static_assert(!args_bad(0, 0) && !args_bad(MAX_N, MAX_SEG) && args_bad(MAX_N + 1, 0) && args_bad(1, MAX_SEG + 1) && !args_bad(0, 5) && !args_bad(5, 0),
                  "args_bad");
    std::vector<size_t> sizes = {0, 1, 2, 31, 63, 64, 65, MAX_N - 1, MAX_N};
    for (size_t pw = msm::RUN; pw <= MAX_N; pw *= msm::RUN)
        for (size_t d = 0; d < 3; d++) sizes.push_back(pw - 1 + d);      // 32^k - 1, 32^k, 32^k + 1
    for (size_t t = msm::RUN; t <= MAX_N; t *= msm::RUN / 2)             // 32 * 16^k: where the sum gains a level (two partials per run of 32)
        for (size_t d = 0; d < 3; d++) sizes.push_back(t - 1 + d);
    for (size_t n : sizes) {
        if (n > MAX_N) continue;
        const Plan p = make_plan(n);
        assert(p.levels <= msm::MAX_LEVELS && drive(n, p) == p.levels);
        int want = 0;
        for (size_t v = n; v; v = v <= msm::RUN ? 0 : 2 * msm::runs_of((uint32_t)v)) want++;
        assert(p.levels == want);
        if (n) assert(p.level_in[p.levels - 1] <= msm::RUN && (p.levels == 1 || p.level_in[p.levels - 2] > msm::RUN));
    }
    assert(make_plan(32).levels == 1 && make_plan(33).levels == 2 && make_plan(512).levels == 2 && make_plan(513).levels == 3);
    assert(make_plan(8192).levels == 3 && make_plan(8193).levels == 4 && make_plan(MAX_N).levels == 6);
    const size_t segs[] = {0, 1, 63, 64, 65, 256, MAX_SEG};
    for (size_t n : sizes)
        for (size_t n_seg : segs)
            for (int verify = 0; verify < 2; verify++) {
                if (args_bad(n, n_seg)) continue;
                const Plan p = make_plan(n);
                const Layout L = layout(n, n_seg, verify != 0);
                const size_t o[] = {L.word,   L.sums,    L.keys,   L.jrec, L.part_k[0], L.part_j[0], L.part_k[1], L.part_j[1], L.flag,  L.sc, L.st,
                                    L.apk,    L.apk_inf, L.apk_st, L.hq,   L.hinf,      L.neg_g1,    L.neg_g1_inf, L.s,        L.s_inf, L.ml, L.total};
                const int no = (int)(sizeof o / sizeof o[0]);
                for (int i = 0; i + 1 < no; i++) assert(o[i] % 256 == 0 && o[i] <= o[i + 1]);
                assert(L.word == 0 && L.sums == 256 && L.fill == 256 + n_seg * 192 && L.fill % 16 == 0 && L.word + L.fill <= L.keys);
                assert(L.jrec - L.keys >= n * 4 && L.part_k[0] - L.jrec >= n * 192);
                for (int i = 0; i < 2; i++) {
                    assert(L.part_j[i] - L.part_k[i] >= (size_t)p.part_cap[i] * 4);
                    assert((i ? L.flag : L.part_k[1]) - L.part_j[i] >= (size_t)p.part_cap[i] * 192);
                }
                if (verify) {
                    assert(L.sc - L.flag >= 8 && L.st - L.sc >= n * 32 && L.apk - L.st >= 2 * n);
                    assert(L.apk_inf - L.apk >= 96 * n_seg && L.apk_st - L.apk_inf >= n_seg && L.hq - L.apk_st >= n_seg);
                    assert(L.hinf - L.hq >= 192 * n_seg && L.neg_g1 - L.hinf >= n_seg && L.neg_g1_inf - L.neg_g1 >= 96 && L.s - L.neg_g1_inf >= 1);
                    assert(L.s_inf - L.s >= 192 && L.ml - L.s_inf >= 1 && L.total - L.ml >= 3 * 576);
                } else {
                    assert(L.total == L.flag);
                }
                assert(L.total < ((size_t)1 << 36));
            }
    // the host flavour's refusal
    const uint64_t good[] = {0, 0, 3, 3, 5}, dec[] = {0, 4, 3, 5, 5}, first[] = {1, 1, 3, 3, 5}, beyond[] = {0, 0, 3, 3, 6}, below[] = {0, 0, 3, 3, 4};
    assert(!offsets_malformed(good, 4, 5) && offsets_malformed(dec, 4, 5) && offsets_malformed(first, 4, 5) && offsets_malformed(beyond, 4, 5) &&
           offsets_malformed(below, 4, 5));
    const uint64_t none[] = {0}, huge[] = {0, (uint64_t)1 << 63, 5};
    assert(!offsets_malformed(none, 0, 0) && offsets_malformed(none, 0, 1) && offsets_malformed(huge, 2, 5));
    std::puts("ok");
    return 0;
}
