// zkp_miller1_lanes.hpp -- the lane constants of k_miller1 (zkp_coop.hip) and the test that lets a launch take that kernel: PURE
// arithmetic, no HIP type, no allocation, no I/O.  zkp_coop.hip compiles this text for the device (the kernel's entry) and for the host
// (run_prog, miller_on_pipe); tests/miller1_plan_check.cpp compiles it with g++ -fsanitize=address,undefined, prints the constants of
// a launch for tests/test_miller1_cpu.py (the emulated wavefront starts from them) and walks the predicate at its edges.
//
// A wavefront works on GROUPS = 5 checks, twelve lanes each (lanes 60..63 own nothing).  Lane `lig` of group `grp`:
//   vgb    LDS byte address of the group's slots (the constants come first: SC records per plane)
//   vdst   the lane's result slot; its companion slot is twelve records on
//   vtab   the lane's entry inside a row of the operand table (8 bytes: A1, B1)
//   voff   byte offset, inside one line step, of the half record of line coefficient lig / 2 the lane fetches
//   vland  LDS byte address where that half record lands (line slots 24..29; the second half two planes on)
//   vst    byte offset of the lane's state record: element lig + st_off of check `check` in a buffer of nc checks
// All offsets are 32-bit in the kernel: eligible() is the condition under which none of them wraps.
#pragma once
#include <stdint.h>

#include "zkp_miller1.inc"

#if defined(__HIPCC__)
#define ZKP_M1_HD __host__ __device__ __forceinline__
#else
#define ZKP_M1_HD inline
#endif

namespace zkp {
namespace m1 {

constexpr uint32_t GROUPS = 5, LIG = 12;
constexpr uint32_t S = ZKP_MILLER1_S, SC = ZKP_MILLER1_SC, PS = ZKP_MILLER1_PS, SG = (PS - SC) / GROUPS;
constexpr uint32_t LINE_SLOT = ZKP_MILLER1_LINE_SLOT, LINE_STEPS = ZKP_MILLER1_LINE_STEPS;
static_assert(SC + GROUPS * SG == PS && SG >= S + 6, "a plane: the constants, then five groups of S slots and at least six padding records");

struct Lanes {
    uint32_t grp, lig, check;
    uint32_t vgb, vdst, vtab, voff, vland, vst;
};

// lane < GROUPS * LIG; n_checks: the checks of the launch (the stride of the line buffer), nc: the checks of the state buffer
ZKP_M1_HD Lanes lanes(int lane, uint32_t block, uint32_t n_checks, uint32_t nc, uint32_t st_off) {
    Lanes c;
    const int grp = (lane * 43) >> 9, lig = lane - grp * (int)LIG;
    c.grp = (uint32_t)grp;
    c.lig = (uint32_t)lig;
    c.check = block * GROUPS + grp;
    const uint32_t half = lig & 1, coef = lig >> 1;        // the lane fetches half a record of line coefficient `coef`
    c.vgb = 16u * (SC + grp * SG);
    c.vdst = c.vgb + 16u * lig;
    c.vtab = 8u * lig;
    c.voff = (coef * n_checks + c.check) * 64u + half * 32u;
    c.vland = c.vgb + 16u * (LINE_SLOT + coef) + half * (2u * PS * 16u);
    c.vst = ((lig + st_off) * nc + c.check) * 64u;
    return c;
}

// bytes per line step (k = 1): six records of every check
ZKP_M1_HD uint32_t stride(uint32_t n_checks) { return 6u * 64u * n_checks; }

// the 32-bit byte offsets of the kernel reach every line record of n_checks checks and the twelve Miller elements (from st_off on) of a
// state buffer of nc checks: neither buffer goes beyond 4 GB
constexpr bool eligible(uint64_t n_checks, uint64_t nc, uint64_t st_off) {
    return !(n_checks * 6 * 64 * LINE_STEPS >> 32) && !((LIG + st_off) * nc * 64 >> 32);
}

}  // namespace m1
}  // namespace zkp
