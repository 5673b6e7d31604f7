// miller1_plan_check.cpp -- zkvm_pairings_amd/csrc/zkp_miller1_lanes.hpp (the lane constants of k_miller1 and the test that lets a launch
// take that kernel) on the host: a stand-alone program, built by tests/test_miller1_cpu.py with g++ -fsanitize=address,undefined.
//
//   miller1_plan_check                                   the walk; prints "miller1 plan_check ok: <cases> cases"
//   miller1_plan_check <block> <n_checks> <nc> <st_off>  prints "stride <bytes>", "eligible <0|1>" and, for each of the sixty lanes,
//                                                        "lane grp lig check active vgb vdst vtab voff vland vst"
//
// The walk: the predicate at its two edges (the line buffer: 164482 checks fit 4 GB, 164483 do not; the state buffer likewise for
// every offset of the first Miller element), and wherever it accepts, every 32-bit offset of every lane that has a check equals the
// same expression in 64 bits, and the last byte a lane touches lies inside its buffer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../zkvm_pairings_amd/csrc/zkp_miller1_lanes.hpp"

namespace m1 = zkp::m1;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            fprintf(stderr, "miller1_plan_check: %s failed at line %d\n", #c, __LINE__); \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

static size_t g_cases = 0;

// every lane of one wavefront of an accepted launch
static void walk_block(uint32_t block, uint32_t n_checks, uint32_t nc, uint32_t st_off) {
    CHECK(m1::eligible(n_checks, nc, st_off) && n_checks <= nc);
    const uint64_t line_bytes = (uint64_t)n_checks * 6 * 64 * m1::LINE_STEPS, state_bytes = (uint64_t)(m1::LIG + st_off) * nc * 64;
    CHECK((uint64_t)m1::stride(n_checks) == (uint64_t)n_checks * 384);
    for (int lane = 0; lane < (int)(m1::GROUPS * m1::LIG); lane++) {
        const m1::Lanes c = m1::lanes(lane, block, n_checks, nc, st_off);
        CHECK(c.grp == (uint32_t)lane / m1::LIG && c.lig == (uint32_t)lane % m1::LIG && c.check == block * m1::GROUPS + c.grp);
        // LDS: the lane's slots lie in its own group, the landing address in the line slots of that group
        CHECK(c.vgb == 16 * (m1::SC + c.grp * m1::SG) && c.vdst == c.vgb + 16 * c.lig && c.vtab == 8 * c.lig);
        CHECK(c.vland >= c.vgb + 16 * m1::LINE_SLOT && c.vland % (m1::PS * 16) < c.vgb + 16 * m1::S);
        if (c.check >= n_checks) continue;      // the lane has no check: EXEC keeps it from every global access
        const uint64_t coef = c.lig >> 1, half = c.lig & 1;
        const uint64_t voff = (coef * n_checks + c.check) * 64 + half * 32, vst = ((uint64_t)(c.lig + st_off) * nc + c.check) * 64;
        CHECK(voff == c.voff && vst == c.vst);
        CHECK((m1::LINE_STEPS - 1) * (uint64_t)m1::stride(n_checks) + voff + 32 <= line_bytes);
        CHECK(vst + 64 <= state_bytes);
        g_cases++;
    }
}

static void walk() {
    // the line buffer: n * 6 * 64 * 68 bytes
    const uint32_t n_edge = 164482;
    CHECK(m1::LINE_STEPS == 68);
    CHECK(m1::eligible(n_edge, n_edge, 0) && !m1::eligible(n_edge + 1, n_edge + 1, 0));
    CHECK(m1::eligible(1, 1, 0) && !m1::eligible(0xffffffffu, 1, 0));
    for (uint32_t st_off : {0u, 2u, 12u, 24u}) {
        // the state buffer: (12 + st_off) * nc * 64 bytes
        const uint32_t nc_edge = (uint32_t)((((uint64_t)1 << 32) - 1) / (64 * (m1::LIG + st_off)));
        CHECK(m1::eligible(1, nc_edge, st_off) && !m1::eligible(1, nc_edge + 1, st_off));
        CHECK(!m1::eligible(1, 0xffffffffu, st_off));
        for (uint32_t n : {1u, 4u, 5u, 6u, 59u, 60u, 61u, n_edge - 1, n_edge}) {
            for (uint32_t nc : {n, n + 7, nc_edge}) {
                const uint32_t blocks = (n + m1::GROUPS - 1) / m1::GROUPS;
                for (uint32_t block : {0u, blocks / 2, blocks - 1}) walk_block(block, n, nc, st_off);
            }
        }
    }
}

int main(int argc, char** argv) {
    if (argc == 1) {
        walk();
        printf("miller1 plan_check ok: %zu cases\n", g_cases);
        return 0;
    }
    if (argc != 5) {
        fprintf(stderr, "usage: miller1_plan_check [<block> <n_checks> <nc> <st_off>]\n");
        return 2;
    }
    const uint32_t block = (uint32_t)strtoul(argv[1], nullptr, 0), n_checks = (uint32_t)strtoul(argv[2], nullptr, 0);
    const uint32_t nc = (uint32_t)strtoul(argv[3], nullptr, 0), st_off = (uint32_t)strtoul(argv[4], nullptr, 0);
    printf("stride %u\neligible %d\n", m1::stride(n_checks), (int)m1::eligible(n_checks, nc, st_off));
    for (int lane = 0; lane < (int)(m1::GROUPS * m1::LIG); lane++) {
        const m1::Lanes c = m1::lanes(lane, block, n_checks, nc, st_off);
        printf("%d %u %u %u %d %u %u %u %u %u %u\n", lane, c.grp, c.lig, c.check, (int)(c.check < n_checks), c.vgb, c.vdst, c.vtab, c.voff, c.vland,
               c.vst);
    }
    return 0;
}
