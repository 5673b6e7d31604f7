// poly_plan_check.cpp -- the schedule of the batched Fr NTT (zkvm_pairings_amd/csrc/zkp_poly_plan.hpp) replayed on the host: every pass
// of every plan is executed from the planner's index functions and fr::mont_mul alone - the load phase, the rounds of four elements
// per thread through the folded LDS slots, the store phase - the threads of a workgroup one after the other.  tests/test_poly_cpu.py
// builds this with g++ -fsanitize=address,undefined, runs it as a child process and compares the output file, byte for byte, with
// tests/poly_model.py.  Beside the values it checks that each pass reads and writes every element exactly once, that loads and
// stores come in runs of at least four records, that the 32 lanes of a group touch 32 LDS banks, and it walks the planner at the ABI
// maxima.  CPU only: nothing here touches HIP.
//
//   poly_plan_check <in> <out> <t> <kmax>     in: 3 << kmax canonical elements of 32 bytes; out: for k = 0 .. kmax, flags = 0 .. 7,
//                                             n_poly in {1, 3}: the n_poly << k transformed elements
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zkvm_pairings_amd/csrc/zkp_fr.hpp"
#include "../zkvm_pairings_amd/csrc/zkp_kzg_plan.hpp"
#include "../zkvm_pairings_amd/csrc/zkp_poly_plan.hpp"

using namespace zkp;
using fr::NW;

struct E { uint32_t w[NW]; };

[[noreturn]] static void fail(const char* what, unsigned long long a, unsigned long long b, unsigned long long c) {
    std::fprintf(stderr, "poly_plan_check: %s (%llu, %llu, %llu)\n", what, a, b, c);
    std::exit(1);
}
#define REQUIRE(cond, a, b, c) do { if (!(cond)) fail(#cond, (unsigned long long)(a), (unsigned long long)(b), (unsigned long long)(c)); } while (0)

static std::vector<E> g_table;      // w^i, i < 2^g_table_log2, Montgomery form
static unsigned g_table_log2 = 0;
static std::vector<E> g_coset;      // 4 x 2^COSET_LOG2

static void build_tables(unsigned log2_n) {
    constexpr fr::Consts K = fr::make_consts();
    constexpr fr::Roots W = fr::make_roots();
    g_table_log2 = log2_n;
    g_table.resize((size_t)1 << log2_n);
    std::memcpy(g_table[0].w, K.one, 32);
    for (size_t i = 1; i < g_table.size(); i++) fr::mont_mul(g_table[i].w, g_table[i - 1].w, W.omega[log2_n]);
    const uint32_t seven[NW] = {7, 0, 0, 0, 0, 0, 0, 0};
    E g[4];
    fr::to_mont(g[0].w, seven);
    fr::mont_inv(g[2].w, g[0].w);
    for (int which = 0; which < 4; which += 2) {
        g[which + 1] = g[which];
        for (unsigned i = 0; i < poly::COSET_LOG2; i++) fr::mont_mul(g[which + 1].w, g[which + 1].w, g[which + 1].w);
    }
    const size_t n = (size_t)1 << poly::COSET_LOG2;
    g_coset.resize(4 * n);
    for (int which = 0; which < 4; which++) {
        std::memcpy(g_coset[which * n].w, K.one, 32);
        for (size_t j = 1; j < n; j++) fr::mont_mul(g_coset[which * n + j].w, g_coset[which * n + j - 1].w, g[which].w);
    }
}
static void coset_mul(E& x, uint32_t i, uint32_t inv) {
    const uint32_t lo = i & ((1u << poly::COSET_LOG2) - 1), hi = i >> poly::COSET_LOG2;
    fr::mont_mul(x.w, x.w, g_coset[((size_t)(2 * inv) << poly::COSET_LOG2) + lo].w);
    if (hi) fr::mont_mul(x.w, x.w, g_coset[((size_t)(2 * inv + 1) << poly::COSET_LOG2) + hi].w);
}
static void butterfly(bool dit, E& a, E& b, const poly::Pass& P, uint32_t ti) {
    const E& w = g_table[(size_t)ti << (g_table_log2 - P.k)];
    E d;
    if (dit) {
        fr::mont_mul(b.w, b.w, w.w);
        fr::sub(d.w, a.w, b.w);
        fr::add(a.w, a.w, b.w);
        b = d;
    } else {
        fr::sub(d.w, a.w, b.w);
        fr::add(a.w, a.w, b.w);
        fr::mont_mul(b.w, d.w, w.w);
    }
}
// the 32 lanes q0 .. q0 + 31 touch 32 different banks when they access the slots of elements el[0 .. 31]
static void check_banks(const uint32_t* el, const poly::Pass& P, unsigned phase) {
    if (P.t < 7) return;    // a tile of fewer than 32 lanes per group
    uint32_t seen = 0;
    for (int i = 0; i < 32; i++) seen |= 1u << (poly::lds_slot(el[i]) & 31u);
    REQUIRE(seen == 0xffffffffu, P.t, P.lo, phase);
}

static void run_pass(const poly::Pass& P, const std::vector<E>& src, std::vector<E>& dst, size_t n_poly) {
    constexpr fr::Roots W = fr::make_roots();
    const uint32_t tile = 1u << P.t, threads = tile / 4, nmask = poly::low_mask(P.k);
    const size_t tiles = poly::ntt_tiles(n_poly, P.k, P.t);
    REQUIRE(tiles <= 0x7fffffffull, tiles, 0, 0);
    std::vector<uint8_t> rd(P.total, 0), wr(P.total, 0);
    std::vector<E> out(dst.size());
    std::vector<E> sh(tile);
    for (size_t wg = 0; wg < tiles; wg++) {
        for (uint32_t u = 0; u < tile; u++) {
            const uint64_t g = poly::element_index(P, (uint32_t)wg, u);
            if ((u & 3) == 0 && g < P.total)
                for (uint32_t j = 1; j < 4; j++) REQUIRE(poly::element_index(P, (uint32_t)wg, u + j) == g + j, wg, u, j);
            E v;
            std::memset(&v, 0, sizeof v);
            if (g < P.total) {
                rd[g]++;
                v = src[g];
                if (P.coset_in) coset_mul(v, (uint32_t)g & nmask, 0);
            }
            REQUIRE(poly::lds_slot(u) < tile, u, 0, 0);
            sh[poly::lds_slot(u)] = v;
        }
        for (uint32_t r = 0; r < poly::n_rounds(P); r++) {
            const poly::Round R = poly::round_of(P, r);
            REQUIRE(R.pos + 1 < P.t && (R.lo || R.hi), r, R.pos, P.t);
            REQUIRE(!R.lo || (R.pos >= P.cl && R.pos < P.cl + P.kp), r, R.pos, 0);
            REQUIRE(!R.hi || (R.pos + 1 >= P.cl && R.pos + 1 < P.cl + P.kp), r, R.pos, 1);
            for (uint32_t q = 0; q < threads; q++) {
                uint32_t e[4];
                for (uint32_t j = 0; j < 4; j++) {
                    e[j] = poly::round_element(R, q, j);
                    REQUIRE(e[j] < tile, q, j, e[j]);
                }
                if (wg == 0 && (q & 31) == 0 && q + 32 <= threads)
                    for (uint32_t j = 0; j < 4; j++) {
                        uint32_t el[32];
                        for (uint32_t i = 0; i < 32; i++) el[i] = poly::round_element(R, q + i, j);
                        check_banks(el, P, 1 + r);
                    }
                E x0 = sh[poly::lds_slot(e[0])], x1 = sh[poly::lds_slot(e[1])], x2 = sh[poly::lds_slot(e[2])], x3 = sh[poly::lds_slot(e[3])];
                const uint32_t tlo = R.lo ? poly::twiddle_index(P, (uint32_t)wg, e[0], R.pos) : 0;
                const uint32_t th0 = R.hi ? poly::twiddle_index(P, (uint32_t)wg, e[0], R.pos + 1) : 0;
                const uint32_t th1 = R.hi ? poly::twiddle_index(P, (uint32_t)wg, e[1], R.pos + 1) : 0;
                REQUIRE(tlo <= nmask && th0 <= nmask && th1 <= nmask, tlo, th0, th1);
                if (R.lo && P.lo + R.pos == P.cl) REQUIRE(tlo == 0, r, q, tlo);      // the kernel skips this product
                if (P.dit) {
                    if (R.lo) { butterfly(true, x0, x1, P, tlo); butterfly(true, x2, x3, P, tlo); }
                    if (R.hi) { butterfly(true, x0, x2, P, th0); butterfly(true, x1, x3, P, th1); }
                } else {
                    if (R.hi) { butterfly(false, x0, x2, P, th0); butterfly(false, x1, x3, P, th1); }
                    if (R.lo) { butterfly(false, x0, x1, P, tlo); butterfly(false, x2, x3, P, tlo); }
                }
                sh[poly::lds_slot(e[0])] = x0;
                sh[poly::lds_slot(e[1])] = x1;
                sh[poly::lds_slot(e[2])] = x2;
                sh[poly::lds_slot(e[3])] = x3;
            }
        }
        for (uint32_t u = 0; u < tile; u++) {
            uint32_t e;
            uint64_t g;
            poly::store_map(P, (uint32_t)wg, u, &e, &g);
            REQUIRE(e < tile, wg, u, e);
            if ((u & 3) == 0 && g < P.total && (P.store != poly::STORE_BITREV || P.k >= 2))
                for (uint32_t j = 1; j < 4; j++) {
                    uint32_t e2;
                    uint64_t g2;
                    poly::store_map(P, (uint32_t)wg, u + j, &e2, &g2);
                    REQUIRE(g2 == g + j, wg, u, j);
                }
            if (wg == 0 && P.store == poly::STORE_SAME && (u & 31) == 0) {
                uint32_t el[32];
                for (uint32_t i = 0; i < 32; i++) el[i] = u + i;
                check_banks(el, P, 0);
            }
            if (g >= P.total) continue;
            wr[g]++;
            E v = sh[poly::lds_slot(e)];
            if (P.scale) fr::mont_mul(v.w, v.w, W.inv_pow2[P.k]);
            if (P.coset_out) coset_mul(v, (uint32_t)g & nmask, 1);
            out[g] = v;
        }
    }
    for (size_t i = 0; i < P.total; i++) REQUIRE(rd[i] == 1 && wr[i] == 1, i, rd[i], wr[i]);
    dst = out;
}

static std::vector<E> transform(const std::vector<E>& in, size_t n_poly, unsigned k, int flags, unsigned t) {
    const poly::Plan P = poly::make_plan(n_poly, k, flags, t);
    REQUIRE(P.ok && P.n_pass >= 1, k, flags, t);
    REQUIRE(P.workspace == (poly::ntt_workspace_bytes(n_poly, k, flags, t) != 0), k, flags, t);
    if (t == poly::TILE_LOG2) {
        const int want = (flags & poly::NTT_BITREV) ? (k <= 10 ? 1 : k <= 18 ? 2 : 3) : (k <= 10 ? 1 : k <= 16 ? 2 : 3);
        REQUIRE(P.n_pass == want, k, flags, P.n_pass);
    }
    unsigned bits = 0;
    for (int p = 0; p < P.n_pass; p++) {
        const poly::Pass& a = P.pass[p];
        REQUIRE(a.cl + a.kp + a.ch == t && a.k == k && a.t == t, p, a.cl, a.kp);
        REQUIRE(a.lo == 0 || a.cl >= 2, p, a.lo, a.cl);
        REQUIRE(a.kind == poly::KIND_PLACE || (p == P.n_pass - 1 && a.lo == 0 && a.cl == 0 && a.ch == 2 && a.kp + a.ch <= k), p, a.kind, a.ch);
        bits += a.kp;
    }
    REQUIRE(bits == k, bits, k, flags);
    std::vector<E> cur(in.begin(), in.begin() + (n_poly << k)), nxt(cur.size());
    for (int p = 0; p < P.n_pass; p++) {
        run_pass(P.pass[p], cur, nxt, n_poly);
        cur.swap(nxt);
    }
    return cur;
}

static void walk_maxima() {
    using namespace poly;
    const bool lim = !ntt_args_bad(0, 0, 0) && !ntt_args_bad(0, 20, 7) && ntt_args_bad(0, 21, 0) && ntt_args_bad(1, 21, 0) && ntt_args_bad(1, 64, 0) &&
                     ntt_args_bad(1, 0xffffffffu, 0) && !ntt_args_bad((size_t)1 << 26, 0, 0) && ntt_args_bad(((size_t)1 << 26) + 1, 0, 0) &&
                     !ntt_args_bad(64, 20, 0) && ntt_args_bad(65, 20, 0) && ntt_args_bad(1, 1, 8) && ntt_args_bad(1, 1, -1) && ntt_args_bad(SIZE_MAX, 1, 0) &&
                     !open_args_bad(0, 0, 0) && !open_args_bad(16, 20, 1) && open_args_bad(17, 20, 0) && open_args_bad(1, 21, 0) && open_args_bad(1, 1, 2) &&
                     !open_args_bad((size_t)1 << 24, 0, 0) && open_args_bad(((size_t)1 << 24) + 1, 0, 0) && open_args_bad(SIZE_MAX, 3, 0) &&
                     open_args_bad(1, 0xffffffffu, 0);
    REQUIRE(lim, 0, 0, 0);
    for (unsigned k = 0; k <= NTT_MAX_LOG2; k++)
        for (int flags = 0; flags < 8; flags++)
            for (size_t n_poly : {(size_t)1, (size_t)3, NTT_MAX_TOTAL >> k}) {
                const Plan P = make_plan(n_poly, k, flags);
                REQUIRE(P.ok && P.n_pass <= 3, k, flags, n_poly);
                const size_t total = n_poly << k, tiles = ntt_tiles(n_poly, k);
                REQUIRE(total <= NTT_MAX_TOTAL && tiles * 1024 >= total && (tiles - 1) * 1024 < total && tiles <= 65536, k, flags, n_poly);
                REQUIRE(ntt_workspace_bytes(n_poly, k, flags) == ((flags & NTT_BITREV) || k <= 10 ? 0 : total * 32), k, flags, n_poly);
                REQUIRE(ntt_workspace_bytes(n_poly, k, flags) <= (size_t)2 << 30, k, flags, n_poly);
                for (int p = 0; p < P.n_pass; p++) {
                    const Pass& a = P.pass[p];
                    REQUIRE(a.total == total, k, flags, p);
                    // the corners of the grid: the largest index any (workgroup, slot) stands for is the last element
                    uint64_t top = 0;
                    for (uint32_t wg : {(uint32_t)0, (uint32_t)(tiles - 1)})
                        for (uint32_t u : {0u, 1023u}) {
                            uint32_t e;
                            uint64_t g;
                            store_map(a, wg, u, &e, &g);
                            const uint64_t h = element_index(a, wg, u);
                            REQUIRE(e < 1024 && (k <= 10 || (g < total && h < total)), k, flags, p);
                            if (h > top) top = h;
                            if (g > top) top = g;
                        }
                    REQUIRE(top >= total - 1 && top < tiles * 1024, k, flags, top);
                }
            }
    REQUIRE(COSET_BYTES == 131072, COSET_BYTES, 0, 0);
    for (unsigned k = 0; k <= NTT_MAX_LOG2; k++)
        for (size_t n : {(size_t)1, (size_t)5, OPEN_MAX_TERMS >> k}) {
            const size_t slice = open_slice(n, k);
            REQUIRE(slice >= 1 && slice <= n && (slice << k) <= OPEN_SLICE_TERMS, k, n, slice);
            REQUIRE(!kzg::eval_args_bad(slice, k, 0), k, n, slice);
            const kzg::EvalLayout L = kzg::eval_layout(slice, k);
            REQUIRE(L.total <= (slice << k) * 32 + L.inv.total + 256 && L.total <= ((size_t)129 << 20) + 4096, k, n, L.total);
            REQUIRE((n + slice - 1) / slice <= 4, k, n, slice);
        }
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const unsigned t = (unsigned)std::atoi(argv[3]), kmax = (unsigned)std::atoi(argv[4]);
    if (t < 4 || t > 12 || kmax > 16) return 2;
    walk_maxima();
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 3;
    std::vector<E> in((size_t)3 << kmax);
    if (std::fread(in.data(), 32, in.size(), fi) != in.size()) return 3;
    std::fclose(fi);
    build_tables(kmax);
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 3;
    unsigned long long cases = 0;
    for (unsigned k = 0; k <= kmax; k++)
        for (int flags = 0; flags < 8; flags++)
            for (size_t n_poly : {(size_t)1, (size_t)3}) {
                const std::vector<E> out = transform(in, n_poly, k, flags, t);
                if (std::fwrite(out.data(), 32, out.size(), fo) != out.size()) return 3;
                cases++;
            }
    std::fclose(fo);
    std::printf("poly plan_check ok: %llu cases\n", cases);
    return 0;
}
