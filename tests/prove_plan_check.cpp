// prove_plan_check.cpp -- the planner of the Fr sparse product, the QAP quotient and the Groth16 prover
// (zkvm_pairings_amd/csrc/zkp_prove_plan.hpp) walked on the host up to the ABI maxima.  tests/test_prove_cpu.py builds this with
// g++ -fsanitize=address,undefined and runs it as a child process.  It checks that every (nnz, n_rows) gives a lane count 2^t with
// t in 0 .. 6 and that t is the smallest with 2^t >= ceil(nnz / n_rows); that the grid of a product gives every output slot to
// exactly one lane group (its lane 0 writes it) and no slot beyond out_stride to any; that the vectors are covered exactly once by
// the strided y dimension; that the slices of a call cover 0 .. n exactly once and respect the term limit; that the workspace
// regions are 256-byte aligned, do not overlap and end at `total`; and the argument limits at their edges.  CPU only: nothing here
// touches HIP.
//
//   prove_plan_check                       the walk; prints "prove plan_check ok: <cases> cases"
//   prove_plan_check t <nnz> <n_rows> ...  prints the t of each (nnz, n_rows) pair, one per line
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../zkvm_pairings_amd/csrc/zkp_prove_plan.hpp"

using namespace zkp;

[[noreturn]] static void fail(const char* what, unsigned long long a, unsigned long long b, unsigned long long c) {
    std::fprintf(stderr, "prove_plan_check: %s (%llu, %llu, %llu)\n", what, a, b, c);
    std::exit(1);
}
#define REQUIRE(cond, a, b, c) do { if (!(cond)) fail(#cond, (unsigned long long)(a), (unsigned long long)(b), (unsigned long long)(c)); } while (0)

static unsigned long long g_cases = 0;

static std::vector<size_t> edges(size_t max) {
    std::vector<size_t> v = {0, 1, 2, 3};
    for (size_t p = 4; p <= max && p; p <<= 1) {
        v.push_back(p - 1);
        v.push_back(p);
        if (p + 1 <= max) v.push_back(p + 1);
    }
    v.push_back(max);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    while (!v.empty() && v.back() > max) v.pop_back();
    return v;
}

static void check_t() {
    for (size_t nnz : edges(prove::MAX_NNZ))
        for (size_t n_rows : edges(prove::MAX_STRIDE)) {
            const unsigned t = prove::spmv_t(nnz, n_rows);
            REQUIRE(t <= prove::MAX_T, nnz, n_rows, t);
            const size_t mean = n_rows ? (nnz + n_rows - 1) / n_rows : 0;
            REQUIRE(t == prove::MAX_T || ((size_t)1 << t) >= mean, nnz, n_rows, t);
            REQUIRE(t == 0 || ((size_t)1 << (t - 1)) < mean, nnz, n_rows, t);
            g_cases++;
        }
}

// every output slot below out_stride belongs to lane 0 of exactly one lane group; the walk runs the grid's threads
static void check_rows(size_t nnz, size_t n_rows, size_t out_stride) {
    const prove::SpmvGrid g = prove::spmv_grid(nnz, n_rows, 1, out_stride);
    REQUIRE(g.t <= prove::MAX_T && g.y >= 1 && g.y <= prove::MAX_GRID_Y, nnz, n_rows, g.t);
    REQUIRE((unsigned long long)g.x * (prove::TPB >> g.t) >= out_stride, g.x, g.t, out_stride);
    std::vector<unsigned char> owner(out_stride, 0);
    for (uint32_t wg = 0; wg < g.x; wg++)
        for (uint32_t th = 0; th < prove::TPB; th++) {
            const uint32_t k = prove::spmv_row(wg, th, g.t), li = prove::spmv_lane(th, g.t);
            REQUIRE(li < (1u << g.t), wg, th, li);
            if (th) REQUIRE(k == prove::spmv_row(wg, th - 1, g.t) + (li == 0 ? 1u : 0u), wg, th, k);   // adjacent groups, adjacent rows
            if (li == 0 && k < out_stride) owner[k]++;
        }
    for (size_t k = 0; k < out_stride; k++) REQUIRE(owner[k] == 1, k, owner[k], out_stride);
    g_cases++;
}
// the vectors: the grid's y dimension strides them
static void check_vectors(size_t nnz, size_t n_rows, size_t n, size_t out_stride) {
    const prove::SpmvGrid g = prove::spmv_grid(nnz, n_rows, n, out_stride);
    REQUIRE(g.y >= 1 && g.y <= prove::MAX_GRID_Y, n, g.y, 0);
    std::vector<unsigned char> seen(n, 0);
    for (uint32_t y = 0; y < g.y; y++)
        for (size_t j = y; j < n; j += g.y) seen[j]++;
    for (size_t j = 0; j < n; j++) REQUIRE(seen[j] == 1, j, seen[j], n);
    g_cases++;
}

static void check_bitrev() {
    for (unsigned bits = 1; bits <= 12; bits++) {
        std::vector<unsigned char> hit((size_t)1 << bits, 0);
        for (uint32_t v = 0; v < (1u << bits); v++) {
            const uint32_t r = poly::bitrev(v, bits);
            REQUIRE(r < (1u << bits) && poly::bitrev(r, bits) == v, bits, v, r);
            hit[r]++;
        }
        for (unsigned char h : hit) REQUIRE(h == 1, bits, h, 0);
        g_cases++;
    }
    REQUIRE(poly::bitrev(1, 20) == (1u << 19), 0, 0, 0);
}

static void check_slices(size_t n, size_t m, unsigned log2_n) {
    const size_t S = prove::slice(n, m, log2_n), N = (size_t)1 << log2_n, big = m > N ? m : N;
    if (!n) { REQUIRE(S == 0, n, m, log2_n); return; }
    REQUIRE(S >= 1 && S <= n, n, m, S);
    REQUIRE(S == 1 || S * big <= prove::SLICE_TERMS, S, big, 0);
    REQUIRE(S == n || (S + 1) * big > prove::SLICE_TERMS, S, big, n);   // as large as the limit allows
    size_t covered = 0, count = 0;
    if ((n + S - 1) / S > ((size_t)1 << 16)) { g_cases++; return; }   // the loop below is the driver's: walked where it is short
    for (size_t at = 0; at < n; at += S) {
        const size_t cnt = n - at < S ? n - at : S;
        REQUIRE(at == covered && cnt >= 1, at, covered, cnt);
        covered += cnt;
        count++;
    }
    REQUIRE(covered == n && count == (n + S - 1) / S, covered, n, count);
    g_cases++;
}

static void check_layout(size_t S, size_t m, unsigned log2_n, bool prover) {
    const prove::Layout L = prove::layout(S, m, log2_n, prover);
    const size_t N = (size_t)1 << log2_n;
    std::vector<std::pair<size_t, size_t>> reg;   // offset, bytes
    if (prover) reg.push_back({L.a_ev, S * N * 32});
    reg.push_back({L.b_ev, S * N * 32});
    reg.push_back({L.c_ev, S * N * 32});
    if (prover) {
        reg.push_back({L.l_pts, m * 96});
        reg.push_back({L.l_inf, m});
        reg.push_back({L.h_pts, N * 96});
        reg.push_back({L.h_inf, N});
        reg.push_back({L.sc_r, S * 32});
        reg.push_back({L.sc_s, S * 32});
        reg.push_back({L.sc_nrs, S * 32});
        for (int i = 0; i < 8; i++) { reg.push_back({L.g1[i], S * 96}); reg.push_back({L.g1_inf[i], S}); }
        for (int i = 0; i < 3; i++) { reg.push_back({L.g2[i], S * 192}); reg.push_back({L.g2_inf[i], S}); }
    }
    std::sort(reg.begin(), reg.end());
    size_t end = 0;
    for (const auto& r : reg) {
        REQUIRE(r.first % 256 == 0 && r.first >= end, r.first, end, r.second);
        end = r.first + r.second;
    }
    REQUIRE(end <= L.total && L.total - end < 256, end, L.total, 0);
    g_cases++;
}

static void check_limits() {
    using namespace prove;
    REQUIRE(!spmv_args_bad(MAX_STRIDE, MAX_COLS, MAX_NNZ, MAX_OUT / MAX_STRIDE, MAX_STRIDE), 0, 0, 0);
    REQUIRE(spmv_args_bad(0, MAX_COLS + 1, 0, 1, 1), 0, 0, 1);
    REQUIRE(spmv_args_bad(0, 1, MAX_NNZ + 1, 1, 1), 0, 0, 2);
    REQUIRE(spmv_args_bad(5, 1, 0, 1, 4), 0, 0, 3);                      // out_stride < n_rows
    REQUIRE(spmv_args_bad(1, 1, 0, 1, MAX_STRIDE + 1), 0, 0, 4);
    REQUIRE(spmv_args_bad(1, 1, 0, MAX_OUT / 4 + 1, 4), 0, 0, 5);
    REQUIRE(!spmv_args_bad(0, 1, 0, 0, 0) && !spmv_args_bad(0, 0, 0, 7, 0), 0, 0, 6);
    auto r1 = [](unsigned k, size_t l, size_t rows, size_t m, size_t nnz, size_t n) { return r1cs_args_bad(k, l, rows, m, nnz, rows, m, nnz, rows, m, nnz, n); };
    REQUIRE(!r1(1, 0, 2, 1, 0, 0) && !r1(20, 5, MAX_STRIDE, MAX_COLS, MAX_NNZ, MAX_N), 0, 0, 7);
    REQUIRE(r1(0, 0, 1, 1, 0, 1) && r1(21, 0, 1, 1, 0, 1), 0, 0, 8);
    REQUIRE(r1(3, 0, 9, 10, 0, 1), 0, 0, 9);                              // n_rows > N
    REQUIRE(r1(3, 10, 8, 10, 0, 1) && !r1(3, 9, 8, 10, 0, 1), 0, 0, 10);  // n_inputs + 1 > m
    REQUIRE(r1(3, 0, 8, MAX_COLS + 1, 0, 1) && r1(3, 0, 8, 10, MAX_NNZ + 1, 1) && r1(3, 0, 8, 10, 0, MAX_N + 1), 0, 0, 11);
    REQUIRE(r1cs_args_bad(3, 0, 8, 10, 0, 7, 10, 0, 8, 10, 0, 1) && r1cs_args_bad(3, 0, 8, 10, 0, 8, 11, 0, 8, 10, 0, 1) &&
            r1cs_args_bad(3, 0, 8, 10, 0, 8, 10, 0, 8, 9, 0, 1), 0, 0, 12);  // the three disagree
    g_cases++;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "t")) {
        for (int i = 2; i + 1 < argc; i += 2) std::printf("%u\n", prove::spmv_t(std::strtoull(argv[i], nullptr, 10), std::strtoull(argv[i + 1], nullptr, 10)));
        return 0;
    }
    check_t();
    check_bitrev();
    check_limits();
    const size_t strides[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 4097, 65536, prove::MAX_STRIDE};
    for (size_t stride : strides)
        for (unsigned t = 0; t <= prove::MAX_T; t++) {
            const size_t n_rows = stride - (stride > 2 ? 2 : 0);
            const size_t nnz = n_rows ? n_rows * (((size_t)1 << t) - (t ? ((size_t)1 << (t - 1)) - 1 : 0)) : 0;   // a mean that picks t
            REQUIRE(!prove::spmv_args_bad(n_rows, 1, nnz, 1, stride), nnz, n_rows, stride);
            REQUIRE(!n_rows || prove::spmv_t(nnz, n_rows) == t, nnz, n_rows, t);
            check_rows(nnz, n_rows, stride);
            for (size_t n : {(size_t)1, (size_t)3, (size_t)65535, (size_t)65536, (size_t)70000})
                if (!prove::spmv_args_bad(n_rows, 1, nnz, n, stride)) check_vectors(nnz, n_rows, n, stride);
        }
    for (unsigned k = prove::MIN_LOG2; k <= prove::MAX_LOG2; k++)
        for (size_t m : edges(prove::MAX_COLS)) {
            if (!m) continue;
            for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)4099, (size_t)4100, (size_t)1 << 22, ((size_t)1 << 22) + 1, prove::MAX_N}) {
                check_slices(n, m, k);
                const size_t S = prove::slice(n, m, k);
                if (S) { check_layout(S, m, k, false); check_layout(S, m, k, true); }
            }
        }
    std::printf("prove plan_check ok: %llu cases\n", g_cases);
    return 0;
}
