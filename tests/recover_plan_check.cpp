// recover_plan_check.cpp -- zkvm_pairings_amd/csrc/zkp_recover_plan.hpp walked on the host: a stand-alone program, built by
// tests/test_recover_cpu.py with g++ -fsanitize=address,undefined and run as a child process.  For every (log2_n, log2_l) the ABI admits:
// the argument limits at their edges, the shape (C columns of M positions fit the tile, l = C x groups), the slice length, the
// workspace regions (aligned, disjoint, large enough for what the driver puts there at the largest n), and the column kernel's index
// arithmetic replayed element by element - every load inside the slice's coefficients, every store inside the blob's row and the stores
// of a blob's workgroups a bijection onto its N coefficients, every table index inside its table, the rounds of a transform running each
// of its mu stages exactly once in the order of its decimation.
//   recover_plan_check            the walk; prints "recover plan_check ok: <cases> cases"
//   recover_plan_check shapes     reads "n log2_n log2_l" lines, prints "n log2_n log2_l slice cols groups" for each
//   recover_plan_check tiles      reads "log2_n log2_l" lines, prints "log2_n log2_l mu cl cols groups" as the column kernel receives them
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zkvm_pairings_amd/csrc/zkp_recover_plan.hpp"

using namespace zkp;

#define REQUIRE(c)                                                                       \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            fprintf(stderr, "recover_plan_check: %s failed at line %d\n", #c, __LINE__); \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

static void check_rounds(unsigned mu, unsigned cl, unsigned dit) {
    const poly::Pass P = rec::pass_of(mu, cl, dit);
    std::vector<unsigned> order;
    for (uint32_t r = 0; r < poly::n_rounds(P); r++) {
        const poly::Round R = poly::round_of(P, r);
        REQUIRE(R.pos + 1 < poly::TILE_LOG2);
        if (dit) {
            if (R.lo) order.push_back(R.pos);
            if (R.hi) order.push_back(R.pos + 1);
        } else {
            if (R.hi) order.push_back(R.pos + 1);
            if (R.lo) order.push_back(R.pos);
        }
        // the four elements of the 256 lanes cover the tile once
        std::vector<char> seen(1u << poly::TILE_LOG2, 0);
        for (uint32_t q = 0; q < poly::TPB; q++)
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t e = poly::round_element(R, q, j);
                REQUIRE(e < seen.size() && !seen[e]);
                seen[e] = 1;
            }
    }
    REQUIRE(order.size() == mu);
    for (unsigned s = 0; s < mu; s++) REQUIRE(order[s] == (dit ? cl + s : cl + mu - 1 - s));
}

static size_t check_shape(unsigned log2_n, unsigned log2_l, int flags) {
    size_t cases = 0;
    const rec::Shape s = rec::shape_of(log2_n, log2_l);
    const size_t l = (size_t)1 << log2_l, M = (size_t)1 << s.mu, D = (size_t)1 << s.log2_d, N = (size_t)1 << log2_n;
    REQUIRE(s.log2_d == log2_n + 1 && M * l == D && s.mu >= 1 && s.mu <= rec::MAX_LOG2_M && s.cl + s.mu == poly::TILE_LOG2);
    REQUIRE((size_t)s.cols * s.groups == l && s.cols <= (1u << s.cl) && (size_t)s.cols * M <= ((size_t)1 << poly::TILE_LOG2));
    REQUIRE(s.cols == l || s.cols == (1u << s.cl));
    const size_t n_max = rec::MAX_TOTAL >> s.log2_d;
    REQUIRE(!rec::args_bad(n_max, log2_n, log2_l, flags) && rec::args_bad(n_max + 1, log2_n, log2_l, flags) && !rec::args_bad(0, log2_n, log2_l, flags));
    for (size_t n : {(size_t)1, (size_t)2, rec::slice_of(n_max, log2_n), rec::slice_of(n_max, log2_n) + 3, n_max}) {
        if (n > n_max) continue;
        const rec::Layout L = rec::layout(n, log2_n, log2_l, flags);
        REQUIRE(L.slice >= 1 && L.slice <= n && (L.slice == 1 || (L.slice << s.log2_d) <= rec::SLICE_POINTS));
        REQUIRE(L.slice == n || L.slice == (rec::SLICE_POINTS >> s.log2_d) || (L.slice == 1 && D > rec::SLICE_POINTS));
        const size_t cells = L.slice << s.mu;
        const size_t need[5] = {log2_l ? (L.slice << s.log2_d) * 32 : 0, log2_l ? poly::ntt_workspace_bytes(cells, log2_l, poly::NTT_INVERSE | flags) : 0, cells * 32,
                                cells * 32, cells * 32};
        const size_t at[6] = {L.coef, L.ntt, L.zc, L.zr, L.zs, L.total};
        for (int i = 0; i < 5; i++) REQUIRE(at[i] % 256 == 0 && at[i] + need[i] <= at[i + 1]);
        // what the driver hands to the launchers it borrows: within their own limits
        REQUIRE(!poly::ntt_args_bad(cells, log2_l, poly::NTT_INVERSE | flags) && !poly::ntt_args_bad(L.slice, s.mu, poly::NTT_COSET));
        REQUIRE(poly::make_plan(L.slice, s.mu, 0).ok && !poly::make_plan(L.slice, s.mu, 0).workspace && poly::make_plan(cells, log2_l, poly::NTT_INVERSE | flags).ok);
        REQUIRE(L.slice <= 0x7fffffffu && L.slice * s.groups <= 0x7fffffffu);      // the two grids
        cases++;
    }
    // the column kernel, one blob: table_log2 = log2_d and a larger table
    for (unsigned table_log2 : {s.log2_d, 20u}) {
        const rec::Column a = rec::column_of(log2_n, log2_l, flags, table_log2);
        REQUIRE(a.cols == s.cols && a.groups == s.groups && a.mu == s.mu && a.cl == s.cl && a.log2_d == s.log2_d && a.bitrev == (flags ? 1u : 0u));
        const size_t table = (size_t)1 << table_log2;
        if (N > ((size_t)1 << 14)) continue;          // the element walk: up to N = 2^14, where every M and both column regimes (C = l, C < l) have occurred
        std::vector<char> stored(N, 0), loaded(D, 0);
        const uint32_t cmask = poly::low_mask(a.cl), half = 1u << (a.mu - 1);
        for (uint32_t g = 0; g < a.groups; g++)
            for (uint32_t e = 0; e < (1u << poly::TILE_LOG2); e++) {
                const uint32_t c = e & cmask, p = e >> a.cl;
                REQUIRE(p < M);
                if (c >= a.cols) continue;
                const uint32_t i = g * a.cols + c, m = a.bitrev ? poly::bitrev(p, a.mu) : p;
                REQUIRE(i < l && m < M);
                const size_t src = ((size_t)m << a.log2_l) + i;
                REQUIRE(src < D && !loaded[src]);
                loaded[src] = 1;
                REQUIRE(((size_t)rec::inverse_power(p, i, a.log2_d) << a.tshift_d) < table);
                REQUIRE((((size_t)p * i + rec::inverse_power(p, i, a.log2_d)) & (D - 1)) == 0);
                for (uint32_t b = a.cl; b < poly::TILE_LOG2; b++)
                    for (uint32_t inv = 0; inv < 2; inv++) {
                        const uint32_t ex = rec::twiddle_exp(a.mu, a.cl, e & ~(1u << b), b, inv);
                        REQUIRE(ex < M && ((size_t)ex << a.tshift_m) < table && (inv || ex < M / 2));
                    }
                const uint32_t t = poly::bitrev(p, a.mu);
                REQUIRE(t < M && t < ((size_t)1 << poly::COSET_LOG2));
                if (t < half) {
                    const size_t dst = ((size_t)t << a.log2_l) + i;
                    REQUIRE(dst < N && !stored[dst]);
                    stored[dst] = 1;
                }
            }
        for (size_t i = 0; i < N; i++) REQUIRE(stored[i]);
        for (size_t i = 0; i < D; i++) REQUIRE(loaded[i]);
        cases++;
    }
    check_rounds(s.mu, s.cl, 0);
    check_rounds(s.mu, s.cl, 1);
    return cases + 2;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "shapes")) {
        unsigned long n;
        unsigned log2_n, log2_l;
        while (scanf("%lu %u %u", &n, &log2_n, &log2_l) == 3) {
            if (rec::args_bad(n, log2_n, log2_l, 0) || !n) return 2;
            const rec::Shape s = rec::shape_of(log2_n, log2_l);
            printf("%lu %u %u %zu %u %u\n", n, log2_n, log2_l, rec::layout(n, log2_n, log2_l, 0).slice, s.cols, s.groups);
        }
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "tiles")) {
        unsigned log2_n, log2_l;
        while (scanf("%u %u", &log2_n, &log2_l) == 2) {
            if (rec::args_bad(1, log2_n, log2_l, 0)) return 2;
            const rec::Column a = rec::column_of(log2_n, log2_l, 0, log2_n + 1);
            printf("%u %u %u %u %u %u\n", log2_n, log2_l, a.mu, a.cl, a.cols, a.groups);
        }
        return 0;
    }
    size_t cases = 0;
    for (unsigned log2_n = 0; log2_n <= rec::MAX_LOG2_N + 1; log2_n++)
        for (unsigned log2_l = 0; log2_l <= log2_n + 1; log2_l++)
            for (int flags : {0, (int)poly::NTT_BITREV}) {
                const bool bad = log2_n > 19 || log2_l > log2_n || log2_n + 1 - log2_l > 10;
                REQUIRE(rec::args_bad(1, log2_n, log2_l, flags) == bad);
                if (!bad) cases += check_shape(log2_n, log2_l, flags);
            }
    for (int flags : {1, 3, 4, 8, -1}) REQUIRE(rec::args_bad(1, 4, 2, flags));
    REQUIRE(rec::args_bad(1, 10, 0, 0) && !rec::args_bad(1, 9, 0, 0) && !rec::args_bad(64, 19, 19, 0) && rec::args_bad(65, 19, 19, 0) && !rec::args_bad(2, 19, 10, 2));
    REQUIRE(rec::slice_of(1000, 12) == 256 && rec::slice_of(100, 12) == 100 && rec::slice_of(5, 19) == 2 && rec::slice_of((size_t)1 << 25, 0) == ((size_t)1 << 20));
    printf("recover plan_check ok: %zu cases\n", cases);
    return 0;
}
