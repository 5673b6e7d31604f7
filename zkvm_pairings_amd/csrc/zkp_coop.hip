// zkp_coop.hip -- lane-cooperative kernel family (gfx950): the throughput path of the pairing engine.
//
// Pipeline for a chunk of checks (each check = k pairs sharing one Fp12 accumulator):
//   k_prep_lines   two lanes per PAIR (one per Fp2 coefficient): walks the G2 point through the 68 doubling/addition steps of
//                  the optimal-ate loop (ePrint 2010/354 Alg. 26/27), scales every line by P and
//                  streams (c2, c1*xP, c0*yP) to HBM as 28-bit-limb records (coalesced).
//   k_coop(prog)   one check per GROUP of 12 lanes (5 groups per wavefront); lane j owns Fp12
//                  coefficient j; all tower values live in LDS; a table-driven interpreter executes
//                  the step program generated (and verified on the CPU) by tools/coopgen.py:
//                    MULACC  sum of <=12 products into 64-bit columns, ONE Montgomery reduction
//                    LIN     limb-wise linear combination (no carries), weak normalisation
//                    GLOAD/GSTORE  line stream / per-check state / wire format
//                  the optional epilogue (alpha r + beta E, renormalised) and the companion store
//                  (x0 + x1 / x0 - x1 of the lane pair's Fp2 coefficient, so that later steps fetch their
//                  operand forms ready-made) ride on the MULACC step.
//   k_miller1      the Miller loop of one-pair checks (program miller1_state) as ONE asm block on k_coop's lanes and LDS image: no
//                  interpreter, operand addresses from a table in the image's padding, line records requested one line step ahead.
//   k_batch_inv    batched Fp inversions (Montgomery's trick, up to 32 values per lane, division steps): the single inversion
//                  of the final exponentiation and the six per x-power chain of the decompression.
//   k_ksq          the 63 cyclotomic squarings of an x-power chain in Karabina's compressed form: four lanes per check (one Fp2
//                  product each), 16 checks per wavefront, operands in registers, products exchanged by DPP, snapshots of the
//                  running value at the set bits of |x|.
//   k_kdec_a / _b  decompression of the snapshots (two lanes per snapshot) around one k_batch_inv call.
// Programs: miller{k}_{state|wire}, f12mul_{state|wire|pairs}, fexp_a_{state|wire}, fexp_c0..5, tw_* (zkp_coop_prog.inc).
// Host side: a super-chunk of up to 2^20 checks shares one state buffer; phase A (lines, Miller loop, fexp_a) runs per
// 2^16-check chunk on two HIP streams, then ONE k_batch_inv and the phase C plan (ZKP_FEXP_C_PLAN: six step programs
// alternating with the five x-power chains = k_ksq, k_kdec_a, k_batch_inv, k_kdec_b) cover the super-chunk (two_phase).
//
// Reference anchors: Fp12::mul_by_014 src/fp12.rs:99-111, Fp12::square :173-184, Fp12::invert
// :186-190 (+ src/fp6.rs:291-309, src/fp2.rs:278-296), conjugate :123-125; pairing semantics
// SURVEY.md S6 (src/pairings.rs is empty upstream).
#include "zkp_coop.hpp"
#include "zkp_plan.hpp"
#include "zkp_msm_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zkp_coop_prog.inc"
#include "zkp_fp28.hpp"
#include "zkp_coop_mulacc.inc"   // the MULACC step of k_coop and the squaring of k_ksq as hand-scheduled asm blocks (tools/coopasm.py)
#include "zkp_miller1.inc"       // the Miller loop of one-pair checks (k_miller1) as one asm block (tools/coopasm.py generate_miller1)
#include "zkp_miller1_lanes.hpp" // its lane constants and the 4 GB test of its 32-bit offsets (tests/miller1_plan_check.cpp walks them)
#include "zkp_prep_dbl.inc"      // the doubling / addition steps of k_prep_lines as hand-allocated asm blocks (tools/prepasm.py)
#include "zkp_valid_steps.inc"   // the Jacobian doubling / mixed addition of the subgroup checks as asm blocks (tools/validasm.py)

using namespace zkp28;

namespace {

// one wavefront per k_coop workgroup: five checks of twelve lanes, lanes 60..63 idle.  Sixteen checks on three wavefronts (workgroup
// barriers around every step that touches LDS) were bit-exact and measured: 6.25 % fewer wavefronts, but they
// spent 21 % of their cycles at the barriers - the Miller program alone ran 12 % slower, the 2^20-pair pass the same (256.8 / 256.0 ms)
constexpr int GROUPS = 5;              // checks per workgroup
constexpr int LIG = ZKP_COOP_G;        // 12 lanes per group
constexpr int ST_SIZE = ZKP_COOP_ST_SIZE;
constexpr int NLINES = ZKP_COOP_NLINES;
static_assert(zkp::plan::NLINES == NLINES && zkp::plan::ST_SIZE == ST_SIZE && zkp::plan::GROUPS == GROUPS,
              "zkp_plan.hpp (the host's planning arithmetic, checked under sanitizers on the CPU) follows the generated programs");

enum { OP_END = 0, OP_MULACC = 1, OP_LIN = 2, OP_GLOAD = 3, OP_GSTORE = 4, OP_LOOP = 5, OP_ENDLOOP = 6,
       OP_PLOOP = 7, OP_PENDLOOP = 8 };   // round 5: a loop over the k pairs of the launch (run-time count); its counter offsets the line loads
enum { K_LINE = 0, K_STATE = 1, K_WIRE = 2, K_WIRE2 = 3 };   // K_WIRE2: wire record of check + chk_off

__device__ __constant__ const int32_t K_PBAL[NL] = {ZKP_COOP_P_BAL};

// Round 6: the number of checks a launch works on may live in DEVICE memory (zkp_points_check_batch_dev: the checks whose points are all
// valid are counted on the device and never read back).  A launch is planned on the host for the worst case - n checks from `base` of
// the list on - and every kernel takes min(n, *cnt - base) at its entry; wavefronts behind that leave at once.  cnt == nullptr: n as given.
struct NDev { const uint32_t* cnt; uint32_t base; };
__device__ __forceinline__ uint32_t eff_n(uint32_t n, const NDev& nd) {
    if (!nd.cnt) return n;
    const uint32_t m = *nd.cnt;                 // wave-uniform: a scalar load
    const uint32_t left = m > nd.base ? m - nd.base : 0u;
    return left < n ? left : n;
}

struct CoopArgs {
    const uint32_t* hdr;
    const uint32_t* tbl;
    const uint4* rtbl;       // resolved MULACC table: row (table offset / 12 + term) x 64 lanes of {A1 address, B1 address, A2 | B2 << 16, 0};
                             // the row behind a step's terms holds its per-lane flag words (coop_resolve_table)
    const int4* consts;      // NCONST records of 4 int4
    const int4* lines;       // [(step * k + pair) * 6 + c][check] records of 4 int4
    int4* state;             // [elem][check] records of 4 int4
    const uint64_t* wire_in;  // n_checks x 72
    uint64_t* wire_out;       // n_checks x 72 (may be null)
    uint8_t* ok;              // may be null
    int* all_ok;              // may be null
    uint32_t n_checks;
    uint32_t nc;              // record stride of the state buffer (>= n_checks: a super-chunk's state is shared by its chunks)
    uint32_t k;
    uint32_t S;               // LDS plane stride (int4) of a group region (= the program's slot count)
    uint32_t nconst;          // constants the program references (prefix of the table)
    uint32_t st_off;          // added to every K_STATE element index (where a group's Miller value lands)
    uint32_t chk_off;         // K_WIRE2 loads read the wire record of check + chk_off (product tree)
    NDev nd;                  // device-resident check count (or {nullptr, 0})
};

// ---- LDS access: quad-plane SoA, record = 4 x int4 at off, off+S, off+2S, off+3S
__device__ __forceinline__ void lds_ld(int32_t* x, const int4* lds, int off, int S) {
    int4 v0 = lds[off], v1 = lds[off + S], v2 = lds[off + 2 * S], v3 = lds[off + 3 * S];
    x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w;
    x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
    x[8] = v2.x; x[9] = v2.y; x[10] = v2.z; x[11] = v2.w;
    x[12] = v3.x; x[13] = v3.y;
}
__device__ __forceinline__ void lds_st(int4* lds, int off, int S, const int32_t* x) {
    lds[off] = make_int4(x[0], x[1], x[2], x[3]);
    lds[off + S] = make_int4(x[4], x[5], x[6], x[7]);
    lds[off + 2 * S] = make_int4(x[8], x[9], x[10], x[11]);
    lds[off + 3 * S] = make_int4(x[12], x[13], 0, 0);
}

// value renormalisation (tools/coopgen.py vred): q = round(top / p_top); x -= q p; weak_norm
__device__ __forceinline__ void vred(int32_t* x) {
    int32_t q = ((x[NL - 1] >> ZKP_COOP_VRED_SHIFT_IN) * ZKP_COOP_VRED_C + (1 << (ZKP_COOP_VRED_SHIFT_OUT - 1))) >> ZKP_COOP_VRED_SHIFT_OUT;
#pragma unroll
    for (int i = 0; i < NL; i++) x[i] -= q * K_PBAL[i];
    weak_norm(x);
}

__device__ __forceinline__ int sext4(uint32_t v) { return ((int32_t)(v << 28)) >> 28; }
__device__ __forceinline__ int sext8(uint32_t v) { return ((int32_t)(v << 24)) >> 24; }

// canonical [0,p) unsigned 28-bit limbs from a reduced value in (-p, 2p) given as balanced limbs
__device__ __forceinline__ void canon28(uint32_t* f, const int32_t* x) {
    int32_t u[NL], y[NL], z[NL];
    int32_t carry = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        int32_t v = x[i] + carry;
        if (i < NL - 1) { u[i] = v & MASK; carry = v >> W; } else u[i] = v;
    }
    carry = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        int32_t v = u[i] - K28_P[i] + carry;
        if (i < NL - 1) { y[i] = v & MASK; carry = v >> W; } else y[i] = v;
    }
    carry = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        int32_t v = u[i] + K28_P[i] + carry;
        if (i < NL - 1) { z[i] = v & MASK; carry = v >> W; } else z[i] = v;
    }
    bool neg = u[NL - 1] < 0, ge = y[NL - 1] >= 0;
#pragma unroll
    for (int i = 0; i < NL; i++) f[i] = (uint32_t)(neg ? z[i] : (ge ? y[i] : u[i]));
}

__host__ __device__ constexpr int coop_group_stride(int S) { return S + ((4 - S % 8) + 8) % 8; }
constexpr int coop_cfg_slots(uint32_t cfg) { return cfg == 2 ? ZKP_COOP_DEEP_NSLOT : cfg == 1 ? ZKP_COOP_WIDE_NSLOT : ZKP_COOP_NSLOT; }
constexpr int coop_cfg_consts(uint32_t cfg) { return cfg == 2 ? ZKP_COOP_DEEP_NCONST : cfg == 1 ? ZKP_COOP_WIDE_NCONST : ZKP_COOP_NCONST; }
constexpr size_t coop_lds_bytes(int S, int SC) { return (size_t)4 * (SC + GROUPS * coop_group_stride(S)) * 16; }
// the asm block pins 156 VGPRs (80 Karatsuba accumulators - 147 multiply-adds per product block instead of 196, measured on the 2^20-pair
// pass: 296.5 -> 283.3 ms - and two operand sets); with the per-lane context re-derived per step the kernel needs 166 = 3 waves per SIMD,
// no spills (12 x 11-12 KB of LDS per CU)
constexpr int COOP_WAVES = 3;
// S slots per group and SC constants: two instantiations - <24, 34> for programs that need the whole constants table (11,136 B of
// LDS per wavefront), <30, 4> for the Miller programs (30 slots, 4 constants; 11,776 B); twelve wavefronts per CU either way
template <int S, int SC>
__global__ void __launch_bounds__(64, COOP_WAVES) k_coop(CoopArgs A) {
    extern __shared__ int4 lds[];
    const uint32_t n_checks = eff_n(A.n_checks, A.nd);     // wave-uniform; also the stride of the line buffer (k_prep_lines takes the same)
    if (blockIdx.x * GROUPS >= n_checks) return;          // the whole workgroup: nothing below is reached by part of it
    const int lane = threadIdx.x;
    // per-lane values, all functions of the lane number.  They are re-derived at the top of every step and again behind the asm
    // MULACC block from an opaque copy of `lane` (ZKP_LANE_CTX): kept in registers across the block they would cost the kernel its
    // third wavefront per SIMD (the block owns 156 of the 168 VGPRs)
    int grp, lig, gbase;
    uint32_t check;
    bool lane_ok, active;
    // S, SC: compile-time plane strides (the q * stride offsets fold into the ds_read/ds_write immediates); A.nconst
    // of the SC constants are uploaded
    // LDS image: four planes (limb quads) of PS records; a plane holds the SC constants, then SG records per group.  ONE plane
    // stride for constants and slots: the plane offsets of every ds_read / ds_write are immediates and an operand's address is
    // (its group's base or 0) + its number.  SG = S rounded up to 4 mod 8: the lane groups of a ds_read_b128 (lanes of up to
    // three check groups) then fall on different bank quads for neighbouring slots.
    constexpr int SG = coop_group_stride(S), PS = SC + GROUPS * SG;
#define ZKP_LANE_CTX()                                                                                  \
    do {                                                                                                \
        int l_ = lane;                                                                                  \
        asm volatile("" : "+v"(l_));                                                                    \
        grp = (l_ * 43) >> 9;             /* lane / 12 for lane < 64 */                                 \
        lig = l_ - grp * LIG;                                                                           \
        lane_ok = grp < GROUPS;                                                                         \
        check = blockIdx.x * GROUPS + grp;                                                              \
        active = lane_ok && check < n_checks;                                                           \
        gbase = SC + (lane_ok ? grp : GROUPS - 1) * SG;                                                 \
    } while (0)

    for (int i = lane; i < (int)A.nconst * 4; i += 64) lds[(i & 3) * PS + (i >> 2)] = A.consts[i];
    __syncthreads();
    // lanes 60..63 own nothing (five checks of twelve lanes): they leave here, so that their multiply-adds draw no power.  EXEC never
    // holds them again (every asm block restores the EXEC it was entered with; no DPP or ballot of a live lane reads them: they are a
    // quad of their own).
    if (lane >= GROUPS * LIG) return;
    // the lanes that own a coefficient of a live check: wave-uniform (two SGPRs), the store mask of the asm MULACC block
    ZKP_LANE_CTX();
    const unsigned long long act_lanes = __ballot(active);

    // the step headers are read-only and wave-uniform: through the constant address space they become scalar loads
    // (s_load_dwordx4 into SGPRs, scalar cache) instead of a vector load + readfirstlane per word
    typedef const __attribute__((address_space(4))) uint32_t* chdr_t;
    chdr_t hdr = (chdr_t)(uintptr_t)A.hdr;
    const uint32_t* __restrict__ tbl = A.tbl;
    uint32_t cursor = 0;
    int pc = 0, loop_pc = 0, loop_left = 0;
    int ploop_pc = 0, ploop_left = 0;
    uint32_t pair6 = 0;      // 6 x the pair loop's counter (0 outside a pair loop): wave-uniform
    auto slot_off = [&](uint32_t s) -> int { return ((s & 64) ? 0 : gbase) + (int)(s & 63); };
    auto ld = [&](int32_t* x, uint32_t s) { lds_ld(x, lds, slot_off(s), PS); };

    for (;;) {
        const uint32_t h0 = hdr[4 * pc], h1 = hdr[4 * pc + 1], off = hdr[4 * pc + 2];
        const uint32_t op = h0 & 0xff, arg = (h0 >> 8) & 0xff;
        if (op == OP_END) break;
        ZKP_LANE_CTX();
        if (op == OP_MULACC) {
            const uint32_t h3 = hdr[4 * pc + 3];
            const uint32_t T = arg;
            // one inline-asm block (tools/coopasm.py): term loop on two operand register sets with resolved per-lane LDS
            // addresses, Karatsuba fold, row-pipelined Montgomery reduction, limb extraction
            const uint4* rt = A.rtbl + (size_t)(off / LIG) * 64;
            // round 4: a step without epilogue stores its result and its companion form from inside the block (resolved
            // addresses in the flag row of the table, the active lanes as a mask)
            const uint32_t nost = h1 & 1u;
            int32_t r[NL];
            {
                static_assert(NL == 14, "the generated block is for 14 limbs");
                constexpr uint32_t PL[NL] = {ZKP28_P_LIMBS};
                asm volatile(ZKP_MULACC_ASM
                             : ZKP_MULACC_OUTS(r)
                             : [rt] "s"(rt), [T] "s"(T), [h1] "s"(h1), [h3] "s"(h3), [lane16] "v"(lane * 16),   // (rematerialised from the lane number: not a live value)
                               [act] "s"(act_lanes), [nost] "s"(nost),
                               [ps1] "i"(PS * 16), [ps2] "i"(PS * 32), [ps3] "i"(PS * 48), [row] "i"(1024),
                               [p0] "s"(PL[0]), [p1] "s"(PL[1]), [p2] "s"(PL[2]), [p3] "s"(PL[3]), [p4] "s"(PL[4]), [p5] "s"(PL[5]), [p6] "s"(PL[6]),
                               [p7] "s"(PL[7]), [p8] "s"(PL[8]), [p9] "s"(PL[9]), [p10] "s"(PL[10]), [p11] "s"(PL[11]), [p12] "s"(PL[12]),
                               [p13] "s"(PL[13]), [pinv] "s"(ZKP28_PINV)
                             : ZKP_MULACC_CLOBBERS);
            }
            if (!nost) { pc++; continue; }
            ZKP_LANE_CTX();
            const uint32_t ew = tbl[off + T * LIG + lig];
            if (h1 & 1) {  // step-uniform: epilogue dst = alpha r + beta E, renormalised
                int32_t e[NL];
                ld(e, (ew >> 16) & 127);
                const int32_t al = sext4((ew >> 8) & 15), be = sext4((ew >> 12) & 15);
                // value renormalisation folded in: q = round(value / p) from the top limb of the combination
                // (the lower limbs are normalised: their carries cannot move q), then ONE weak normalisation
                const int32_t top = al * r[NL - 1] + be * e[NL - 1];
                const int32_t q = ((top >> ZKP_COOP_VRED_SHIFT_IN) * ZKP_COOP_VRED_C + (1 << (ZKP_COOP_VRED_SHIFT_OUT - 1))) >> ZKP_COOP_VRED_SHIFT_OUT;
#pragma unroll
                for (int i = 0; i < NL; i++) r[i] = al * r[i] + be * e[i] - q * K_PBAL[i];
                weak_norm(r);
            }
            if (active && ((ew >> 7) & 1)) lds_st(lds, gbase + (int)(ew & 63), PS, r);
            if (h1 & 2) {  // step-uniform: companion store of a squaring run - the even lane of an Fp2 coefficient keeps
                           // x0 + x1, the odd lane x0 - x1, so that the next squaring reads its operand forms ready-made
                int32_t c2[NL];
                const bool odd = lig & 1;
#pragma unroll
                for (int i = 0; i < NL; i++) {
                    const int32_t o = __builtin_amdgcn_update_dpp(0, r[i], 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, false);
                    c2[i] = odd ? o - r[i] : r[i] + o;
                }
                if (active && ((ew >> 29) & 1)) lds_st(lds, gbase + (int)((ew >> 23) & 63), PS, c2);
            }
        } else if (op == OP_LIN) {
            int32_t r[NL];
#pragma unroll
            for (int i = 0; i < NL; i++) r[i] = 0;
#pragma unroll 1
            for (uint32_t t = 0; t < arg; t++) {
                const uint32_t w = tbl[off + t * LIG + lig];
                int32_t x[NL];
                ld(x, w & 127);
                const int32_t c = sext8((w >> 8) & 0xff);
#pragma unroll
                for (int i = 0; i < NL; i++) r[i] += c * x[i];
            }
            weak_norm(r);
            if (h1 & 1) vred(r);   // only where the generator's static value bound asks for it
            const uint32_t ew = tbl[off + arg * LIG + lig];
            if (active && ((ew >> 7) & 1)) lds_st(lds, gbase + (int)(ew & 63), PS, r);
        } else if (op == OP_GLOAD) {
            const uint32_t w = tbl[off + lig];
            const uint32_t idx = w >> 8;
            if (active && ((w >> 7) & 1)) {
                int32_t x[NL];
                if (arg == K_WIRE || arg == K_WIRE2) {
                    const uint64_t* src = A.wire_in + ((size_t)check + (arg == K_WIRE2 ? A.chk_off : 0u)) * 72 + idx * 6;
                    uint64_t ww[6];
#pragma unroll
                    for (int i = 0; i < 6; i++) ww[i] = src[i];
#pragma unroll
                    for (int i = 0; i < NL; i++) {
                        const int bit = W * i, word = bit >> 6, sh = bit & 63;
                        uint64_t v = ww[word] >> sh;
                        if (sh > 64 - W && word + 1 < 6) v |= ww[word + 1] << (64 - sh);
                        x[i] = (int32_t)(v & (uint64_t)MASK);
                    }
                } else {
                    size_t rec;
                    if (arg == K_LINE) rec = ((size_t)cursor * A.k * 6 + pair6 + idx) * n_checks + check;   // line buffer: this launch's checks only
                    else rec = (size_t)(idx + A.st_off) * A.nc + check;
                    const int4* src = (arg == K_LINE ? A.lines : (const int4*)A.state) + rec * 4;
                    int4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
                    x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
                    x[8] = v2.x; x[9] = v2.y; x[10] = v2.z; x[11] = v2.w; x[12] = v3.x; x[13] = v3.y;
                }
                lds_st(lds, gbase + (int)(w & 63), PS, x);
            }
            cursor += h1;
        } else if (op == OP_GSTORE) {
            const uint32_t w = tbl[off + lig];
            const uint32_t idx = w >> 8;
            const bool part = active && ((w >> 7) & 1);
            int32_t x[NL];
            lds_ld(x, lds, gbase + (int)(w & 63), PS);
            if (arg == K_STATE) {
                if (part) {
                    int4* dst = A.state + ((size_t)(idx + A.st_off) * A.nc + check) * 4;
                    dst[0] = make_int4(x[0], x[1], x[2], x[3]);
                    dst[1] = make_int4(x[4], x[5], x[6], x[7]);
                    dst[2] = make_int4(x[8], x[9], x[10], x[11]);
                    dst[3] = make_int4(x[12], x[13], 0, 0);
                }
            } else {
                uint32_t f[NL];
                canon28(f, x);
                if (part && A.wire_out) {
                    uint64_t o[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int i = 0; i < NL; i++) {
                        const int bit = W * i, word = bit >> 6, sh = bit & 63;
                        o[word] |= (uint64_t)f[i] << sh;
                        if (sh > 64 - W && word + 1 < 6) o[word + 1] |= (uint64_t)f[i] >> (64 - sh);
                    }
                    uint64_t* dst = A.wire_out + (size_t)check * 72 + idx * 6;
#pragma unroll
                    for (int i = 0; i < 6; i++) dst[i] = o[i];
                }
                if (h1 & 1) {  // Gt == identity ?  coefficient 0 must be 1, the others 0
                    uint32_t d = f[0] ^ (idx == 0 ? 1u : 0u);
#pragma unroll
                    for (int i = 1; i < NL; i++) d |= f[i];
                    const unsigned long long good = __ballot((d == 0) || !part);
                    const unsigned gm = (unsigned)((good >> (grp * LIG)) & 0xfffu);
                    if (active && lig == 0) {
                        const bool is_one = gm == 0xfffu;
                        if (A.ok) A.ok[check] = is_one ? 1 : 0;
                        if (A.all_ok && !is_one) atomicAnd(A.all_ok, 0);
                    }
                }
            }
        } else if (op == OP_LOOP) {
            loop_pc = pc + 1;
            loop_left = (int)h1;
        } else if (op == OP_ENDLOOP) {
            if (--loop_left > 0) { pc = loop_pc; continue; }
        } else if (op == OP_PLOOP) {
            ploop_pc = pc + 1;
            ploop_left = (int)A.k;
            pair6 = 0;
        } else if (op == OP_PENDLOOP) {
            if (--ploop_left > 0) { pair6 += 6; pc = ploop_pc; continue; }
            pair6 = 0;
            cursor += h1;
        }
        pc++;
    }
}

// =============================================================================== the Miller loop of one-pair checks, uninterpreted
// k_miller1 computes what k_coop<30,4> computes on the program miller1_state (tools/coopgen.py prog_miller(1, False)): same lanes, same
// LDS image, same limbs in every slot and state record.  The whole loop is ONE asm block (tools/coopasm.py generate_miller1): an iteration
// is straight-line code (line product, squaring), its operand addresses come from a table that sits in the padding of the LDS image, and
// the six line records of a step are requested one line step ahead - half a record per lane, into eight landing registers - so that the
// line product and the squaring in between hide their latency; the interpreter's GLOAD step (two dependent memory waits in the
// wavefront's only instruction stream, then a staging copy through fourteen registers) is gone.  ZKP_COOP_MILLER1=0 selects the
// interpreter again (cross-check, A/B).
__device__ __constant__ const uint32_t K_M1_TABLE[ZKP_MILLER1_ROWS * LIG * 2] = {ZKP_MILLER1_TABLE};
__device__ __constant__ const uint32_t K_M1_FLAGS[LIG] = {ZKP_MILLER1_FLAGS};

__global__ void __launch_bounds__(64, COOP_WAVES) k_miller1(CoopArgs A) {
    extern __shared__ int4 lds[];
    constexpr int S = ZKP_COOP_WIDE_NSLOT, SC = ZKP_COOP_WIDE_NCONST, SG = coop_group_stride(S), PS = SC + GROUPS * SG;
    static_assert(S == ZKP_MILLER1_S && SC == ZKP_MILLER1_SC && PS == ZKP_MILLER1_PS && NLINES == ZKP_MILLER1_LINE_STEPS && NL == 14 && LIG == 12,
                  "the generated block is for the <30, 4> image of the Miller programs");
    static_assert(SG - S >= 6 && ZKP_MILLER1_ROWS <= 4 * GROUPS, "a table row takes the six padding records of one group in one plane");
    static_assert(zkp::m1::SG == SG && zkp::m1::GROUPS == GROUPS && zkp::m1::LIG == LIG && zkp::m1::LINE_STEPS == NLINES,
                  "zkp_miller1_lanes.hpp describes this kernel's lanes");
    const uint32_t n_checks = eff_n(A.n_checks, A.nd);     // also the stride of the line buffer (k_prep_lines takes the same)
    if (blockIdx.x * GROUPS >= n_checks) return;
    const int lane = threadIdx.x;
    for (int i = lane; i < (int)A.nconst * 4; i += 64) lds[(i & 3) * PS + (i >> 2)] = A.consts[i];
    // operand table: row r = twelve lanes x (A1, B1) in the padding records of plane r / 5, group r % 5
    uint32_t* const lds32 = (uint32_t*)lds;
    for (int i = lane; i < ZKP_MILLER1_ROWS * LIG * 2; i += 64) {
        const int r = i / (LIG * 2), w = i - r * (LIG * 2);
        lds32[4 * ((r / GROUPS) * PS + SC + (r % GROUPS) * SG + S) + w] = K_M1_TABLE[i];
    }
    __syncthreads();
    if (lane >= GROUPS * LIG) return;      // as in k_coop: lanes 60..63 own nothing
    // the lane constants (zkp_miller1_lanes.hpp: the same text runs on the host, under sanitizers, and feeds the emulated wavefront)
    const zkp::m1::Lanes c = zkp::m1::lanes(lane, blockIdx.x, n_checks, A.nc, A.st_off);
    const unsigned long long act_lanes = __ballot(c.check < n_checks);
    const uint32_t flags = K_M1_FLAGS[c.lig];
    const uint32_t stride = zkp::m1::stride(n_checks);     // bytes per line step (k = 1)
    constexpr uint32_t PL[NL] = {ZKP28_P_LIMBS};
    asm volatile(ZKP_MILLER1_ASM
                 :
                 : ZKP_MILLER1_INS(c.vtab, c.vgb, flags, c.vdst, c.voff, c.vland, c.vst),
                   [lines] "s"(A.lines), [state] "s"(A.state), [stride] "s"(stride), [act] "s"(act_lanes),
                   [p0] "s"(PL[0]), [p1] "s"(PL[1]), [p2] "s"(PL[2]), [p3] "s"(PL[3]), [p4] "s"(PL[4]), [p5] "s"(PL[5]), [p6] "s"(PL[6]),
                   [p7] "s"(PL[7]), [p8] "s"(PL[8]), [p9] "s"(PL[9]), [p10] "s"(PL[10]), [p11] "s"(PL[11]), [p12] "s"(PL[12]),
                   [p13] "s"(PL[13]), [pinv] "s"(ZKP28_PINV)
                 : ZKP_MILLER1_CLOBBERS);
}

// =============================================================================== thread-level Fp28 helpers
__device__ __forceinline__ void f_add(Fp28& r, const Fp28& a, const Fp28& b) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = a.l[i] + b.l[i];
    weak_norm(r.l);
}
__device__ __forceinline__ void f_sub(Fp28& r, const Fp28& a, const Fp28& b) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = a.l[i] - b.l[i];
    weak_norm(r.l);
}
__device__ __forceinline__ void f_set(Fp28& r, const int32_t* k) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = k[i];
}
__device__ __forceinline__ void f_zero(Fp28& r) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = 0;
}

__device__ __forceinline__ void rec_store(int4* dst, const Fp28& x) {
    dst[0] = make_int4(x.l[0], x.l[1], x.l[2], x.l[3]);
    dst[1] = make_int4(x.l[4], x.l[5], x.l[6], x.l[7]);
    dst[2] = make_int4(x.l[8], x.l[9], x.l[10], x.l[11]);
    dst[3] = make_int4(x.l[12], x.l[13], 0, 0);
}
__device__ __forceinline__ void rec_load(Fp28& x, const int4* src) {
    int4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
    x.l[0] = v0.x; x.l[1] = v0.y; x.l[2] = v0.z; x.l[3] = v0.w; x.l[4] = v1.x; x.l[5] = v1.y; x.l[6] = v1.z; x.l[7] = v1.w;
    x.l[8] = v2.x; x.l[9] = v2.y; x.l[10] = v2.z; x.l[11] = v2.w; x.l[12] = v3.x; x.l[13] = v3.y;
}

// =============================================================================== compressed squaring runs: four lanes per check
// The hard part of the final exponentiation is five exponentiations by |x| of values in the cyclotomic subgroup: 63
// squarings each.  In the interpreter a squaring costs 36 product blocks + 12 reductions on twelve lanes (Granger-Scott,
// every output coefficient recomputes the Fp2 squares it shares with its neighbour).  Karabina's compressed form
// (ePrint 2010/542) keeps four of the six Fp2 coefficients, z2..z5 of
//     g = (z0 + z1 s) + (z2 + z3 s) w + (z4 + z5 s) w^2,   s = w^3, s^2 = xi
// (tower positions: z0 c0.c0, z4 c0.c1, z3 c0.c2, z2 c1.c0, z1 c1.c1, z5 c1.c2), and the Granger-Scott recurrences of
// those four need only themselves:
//     z2' = 6 xi B45 + 2 z2          z3' = 3 (A45 - (1 + xi) B45) - 2 z3        A45 = (z4 + z5)(z4 + xi z5), B45 = z4 z5
//     z4' = 3 (A23 - (1 + xi) B23) - 2 z4          z5' = 6 B23 + 2 z5           A23 = (z2 + z3)(z2 + xi z3), B23 = z2 z3
// FOUR Fp2 products per squaring.  k_ksq gives each to one lane (4 product blocks + 2 reductions per lane, four lanes per
// check, SIXTEEN checks per wavefront, no idle lane), operands in registers, the products exchanged inside the lane quad
// with DPP (no LDS traffic but the parked copy of a lane's own coefficient, no step tables).  An exponentiation by |x| is
// ONE run of 57 squarings that stores a snapshot of (z2..z5) after 16, 48 and 57 squarings (the low set bits of |x|; the
// plan says which - rounds 2-3 ran all 63 with six snapshots); k_kdec_a / k_batch_inv / k_kdec_b recover z0, z1 of the
// snapshots (one shared batched inversion), and the step program squares on uncompressed through bits 60, 62, 63 and
// multiplies the six powers.  tools/coopgen.py emu_ksq / emu_kdec are the limb-exact models of these kernels.
constexpr int KS_CHECKS = 16;
// a squaring of k_ksq behind its operand forms is ONE asm block (tools/coopasm.py generate_ksq): the Fp2 product as Karatsuba terms
// + tail on register operands (980 multiply-adds instead of the 1,204 of two product-scanning multiplies), DPP combinations, both
// carry chains, parking.  The block pins 162 VGPRs (four operands, both results' homes, 78 accumulator registers): three waves per SIMD
constexpr int KSQ_WAVES = 3;

__device__ __forceinline__ void park_st(int4* xch, int lane, const int32_t* re, const int32_t* im) {
    xch[0 * 64 + lane] = make_int4(re[0], re[1], re[2], re[3]);
    xch[1 * 64 + lane] = make_int4(re[4], re[5], re[6], re[7]);
    xch[2 * 64 + lane] = make_int4(re[8], re[9], re[10], re[11]);
    xch[3 * 64 + lane] = make_int4(re[12], re[13], im[0], im[1]);     // re0..re13, im0..im13 as seven quads: the asm body of k_ksq
    xch[4 * 64 + lane] = make_int4(im[2], im[3], im[4], im[5]);       // parks them straight from 28 consecutive registers
    xch[5 * 64 + lane] = make_int4(im[6], im[7], im[8], im[9]);
    xch[6 * 64 + lane] = make_int4(im[10], im[11], im[12], im[13]);
}

// operand forms of a lane's next product, in place: in (x, y) = (the lane's coefficient, its pair partner's).  B lanes: u v =
// mine * partner as they stand.  A lanes: X = u + v and MINUS Y = -(u + xi v), u + xi v = (u0 + v0 - v1) + (u1 + v1 + v0) u with
// v = mine on lane 0, the partner on lane 2 - the asm body wants the A product negated, and here the sign is one operand swap
__device__ __forceinline__ void ksq_forms(int32_t* xr, int32_t* xi, int32_t* yr, int32_t* yi, bool a_lane, bool v_mine) {
    if (a_lane) {
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const int32_t tr = xr[i] + yr[i], ti = xi[i] + yi[i];
            const int32_t vr = v_mine ? xr[i] : yr[i], vi = v_mine ? xi[i] : yi[i];
            xr[i] = tr;
            xi[i] = ti;
            yr[i] = vi - tr;
            yi[i] = -ti - vr;
        }
    }
}
// nsq compressed squarings of the Fp12 value in state elements [elem_in, elem_in + 12) (only z2..z5 are read); after
// squaring number it + 1 where bit it of snap_mask is set, (z2..z5) go to the next snapshot area: 12 elements each from
// elem_snap on, laid out like an Fp12 value whose z0, z1 positions are left for k_kdec_b to fill.
__global__ void __launch_bounds__(64, KSQ_WAVES) k_ksq(int4* state, uint32_t n_checks_in, uint32_t nc, uint32_t elem_in, uint32_t elem_snap,
                                                           uint32_t nsq, uint64_t snap_mask, NDev nd) {
    extern __shared__ int4 parked[];               // 7 x 64 quads, at LDS address 0 (the asm body addresses it by lane number)
    const uint32_t n_checks = eff_n(n_checks_in, nd);
    if (blockIdx.x * KS_CHECKS >= n_checks) return;
    const int lane = threadIdx.x;
    const int r = lane & 3;                        // 0: A23, 1: B23, 2: A45, 3: B45
    const bool b_lane = r & 1;
    const bool mine_is_v = r == 0 || r == 3;       // the lane's own new coefficient: z3' (0), z2' (1), z4' (2), z5' (3)
    const uint32_t check_raw = blockIdx.x * KS_CHECKS + (lane >> 2);
    const bool active = check_raw < n_checks;
    const uint32_t check = active ? check_raw : n_checks - 1;
    const int tu = (r & 2) ? 1 : 3, tv = (r & 2) ? 5 : 2;   // tower positions of the lane's pair (u, v) = (z4, z5) or (z2, z3)
    int4* const st = state + (size_t)check * 4;
    auto rec = [&](uint32_t e) -> int4* { return st + (size_t)e * nc * 4; };

    // X, Y: the two factors of the lane's product.  `mine` is the lane's own coefficient of its pair (u, v) - v on lanes 0
    // and 3, u on lanes 1 and 2 - and `other` the pair partner's.  B lanes: u v = mine * other.  A lanes: (u + v)(u + xi v).
    int32_t xr[NL], xi[NL], yr[NL], yi[NL];
    {
        Fp28 u0, u1, v0, v1;
        rec_load(u0, rec(elem_in + 2 * tu));
        rec_load(u1, rec(elem_in + 2 * tu + 1));
        rec_load(v0, rec(elem_in + 2 * tv));
        rec_load(v1, rec(elem_in + 2 * tv + 1));
        const Fp28 &m0 = mine_is_v ? v0 : u0, &m1 = mine_is_v ? v1 : u1, &o0 = mine_is_v ? u0 : v0, &o1 = mine_is_v ? u1 : v1;
        park_st(parked, lane, m0.l, m1.l);
#pragma unroll
        for (int i = 0; i < NL; i++) { xr[i] = m0.l[i]; xi[i] = m1.l[i]; yr[i] = o0.l[i]; yi[i] = o1.l[i]; }
        ksq_forms(xr, xi, yr, yi, !b_lane, r == 0);
    }
    uint32_t snap = elem_snap;
    // One inline-asm block per squaring (tools/coopasm.py generate_ksq): the Fp2 product, the other pair's products by DPP, the
    // lane-role combinations, both carry chains, the parking of the new coefficient and the pair partner's coefficient by DPP.
    // In: X = xr + xi u, Y = yr + yi u.  Out: the lane's new coefficient in (xr, xi), its partner's in (yr, yi) - the
    // snapshot store and the next product's operand forms stay here.
    static_assert(NL == 14, "the generated block is for 14 limbs");
    {
        constexpr int32_t PB[NL] = {ZKP_KSQ_BODY_P_BAL}, KB[NL] = {ZKP_COOP_P_BAL};
        constexpr int VR[3] = {ZKP_KSQ_BODY_VRED};
        static_assert(VR[0] == ZKP_COOP_VRED_C && VR[1] == ZKP_COOP_VRED_SHIFT_IN && VR[2] == ZKP_COOP_VRED_SHIFT_OUT, "regenerate zkp_coop_mulacc.inc");
        static_assert(PB[0] == KB[0] && PB[1] == KB[1] && PB[5] == KB[5] && PB[12] == KB[12] && PB[13] == KB[13], "regenerate zkp_coop_mulacc.inc");
    }
#pragma unroll 1
    for (uint32_t it = 0; it < nsq; it++) {
        {
            constexpr uint32_t PL[NL] = {ZKP28_P_LIMBS};
            asm volatile(ZKP_KSQ_BODY_ASM
                         : ZKP_KSQ_BODY_IO(xr, xi, yr, yi)
                         : [p0] "s"(PL[0]), [p1] "s"(PL[1]), [p2] "s"(PL[2]), [p3] "s"(PL[3]), [p4] "s"(PL[4]), [p5] "s"(PL[5]), [p6] "s"(PL[6]),
                           [p7] "s"(PL[7]), [p8] "s"(PL[8]), [p9] "s"(PL[9]), [p10] "s"(PL[10]), [p11] "s"(PL[11]), [p12] "s"(PL[12]),
                           [p13] "s"(PL[13]), [pinv] "s"(ZKP28_PINV)
                         : ZKP_KSQ_BODY_CLOBBERS);
        }
        // per-lane values re-derived from an opaque copy of the lane number: kept in registers across the block (which owns 162 of
        // the 168 VGPRs) they would be spilled and reloaded in every squaring
        int l_ = lane;
        asm volatile("" : "+v"(l_));
        const bool a_lane = !(l_ & 1), v_mine = (l_ & 3) == 0;     // lane 0 holds (v, u) = (mine, partner), lane 2 (u, v)
        if (it < 64 && ((snap_mask >> it) & 1)) {      // wave-uniform (a 64-bit shift by 64 or more is undefined)
            const uint32_t chk_ = blockIdx.x * KS_CHECKS + (l_ >> 2);
            int4* const st_ = state + (size_t)(chk_ < n_checks ? chk_ : n_checks - 1) * 4;
            auto rec_ = [&](uint32_t e) -> int4* { return st_ + (size_t)e * nc * 4; };
            const int tu_ = (l_ & 2) ? 1 : 3, tv_ = (l_ & 2) ? 5 : 2;
            if (chk_ < n_checks && a_lane) {
                Fp28 o;
#pragma unroll
                for (int i = 0; i < NL; i++) o.l[i] = xr[i];
                rec_store(rec_(snap + 2 * (v_mine ? tv_ : tu_)), o);
#pragma unroll
                for (int i = 0; i < NL; i++) o.l[i] = xi[i];
                rec_store(rec_(snap + 2 * (v_mine ? tv_ : tu_) + 1), o);
#pragma unroll
                for (int i = 0; i < NL; i++) o.l[i] = yr[i];
                rec_store(rec_(snap + 2 * (v_mine ? tu_ : tv_)), o);
#pragma unroll
                for (int i = 0; i < NL; i++) o.l[i] = yi[i];
                rec_store(rec_(snap + 2 * (v_mine ? tu_ : tv_) + 1), o);
            }
            snap += 12;
        }
        ksq_forms(xr, xi, yr, yi, a_lane, v_mine);
    }
}

// ---- two lanes per pair: lane parity c selects the Fp2 coefficient a value's lane holds ------------------
// An Fp2 value is ONE Fp28 per lane (c = 0: real part, c = 1: imaginary part); add/sub/neg/dbl touch
// only the lane's own coefficient; products fetch the partner's coefficient with a DPP quad swap.
__device__ __forceinline__ void swap_pair(Fp28& o, const Fp28& x) {
#pragma unroll
    for (int i = 0; i < NL; i++) o.l[i] = __builtin_amdgcn_update_dpp(0, x.l[i], 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, false);
}
// The by-value routines multiply in the schoolbook accumulator form (acc_mul).  Measured in round 3: Karatsuba product blocks (147
// multiply-adds instead of 196) cost their callers 29 spilled registers and k_kdec_a / k_kdec_b their third wavefront for no gain; the
// product-scanning multiply cost +0.3 % on the 2^20 pass (at two waves per SIMD its one-column dependency chains are not covered).
// r = coefficient c of (a0 + a1 u)^2 :  c=0: (a0 + a1)(a0 - a1) ;  c=1: (2 a0) a1
// Operands and results travel BY VALUE (VGPRs): with pointers every temporary lives in scratch memory and
// the kernel becomes HBM-bound on its own stack traffic (measured: 50 GB per 2^17 pairs).
__device__ __attribute__((noinline)) Fp28 c_sqr(Fp28 mine, int c) {
    Fp28 o, r;
    swap_pair(o, mine);
    int32_t x[NL], y[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) {
        x[i] = o.l[i] + (c ? o.l[i] : mine.l[i]);
        y[i] = mine.l[i] - (c ? 0 : o.l[i]);
    }
    Acc acc;
    acc_zero(acc);
    acc_mul(acc, x, y);
    acc_reduce(r.l, acc);
    return r;
}
// r = coefficient c of (a0 + a1 u)(b0 + b1 u) :  c=0: a0 b0 - a1 b1 ;  c=1: a0 b1 + a1 b0  (one reduction)
// The second operand of the by-value routines travels as four int4 vectors: clang's AMDGPU ABI passes aggregates in
// registers only while they total at most 16 registers, so a second Fp28 (14 registers) went through the stack - a
// scratch store in the caller and a load the callee had to wait for, at every call.
__device__ __forceinline__ void fp28_unpack(Fp28& x, const int4& q0, const int4& q1, const int4& q2, const int4& q3) {
    x.l[0] = q0.x; x.l[1] = q0.y; x.l[2] = q0.z; x.l[3] = q0.w; x.l[4] = q1.x; x.l[5] = q1.y; x.l[6] = q1.z; x.l[7] = q1.w;
    x.l[8] = q2.x; x.l[9] = q2.y; x.l[10] = q2.z; x.l[11] = q2.w; x.l[12] = q3.x; x.l[13] = q3.y;
}
#define FP28_AS_QUADS(x) make_int4((x).l[0], (x).l[1], (x).l[2], (x).l[3]), make_int4((x).l[4], (x).l[5], (x).l[6], (x).l[7]), \
                         make_int4((x).l[8], (x).l[9], (x).l[10], (x).l[11]), make_int4((x).l[12], (x).l[13], 0, 0)
__device__ __attribute__((noinline)) Fp28 c_mul_q(Fp28 ma, int4 q0, int4 q1, int4 q2, int4 q3, int c) {
    Fp28 mb;
    fp28_unpack(mb, q0, q1, q2, q3);
    Fp28 ao, bo, r;
    swap_pair(ao, ma);
    swap_pair(bo, mb);
    int32_t x1[NL], x2[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) {
        x1[i] = c ? ao.l[i] : ma.l[i];
        x2[i] = c ? ma.l[i] : -ao.l[i];
    }
    Acc acc;
    acc_zero(acc);
    acc_mul(acc, x1, mb.l);
    acc_mul(acc, x2, bo.l);
    acc_reduce(r.l, acc);
    return r;
}
__device__ __forceinline__ Fp28 c_mul(const Fp28& ma, const Fp28& mb, int c) { return c_mul_q(ma, FP28_AS_QUADS(mb), c); }
__device__ __attribute__((noinline)) Fp28 f_mul_q(Fp28 a, int4 q0, int4 q1, int4 q2, int4 q3) {
    Fp28 b, r;
    fp28_unpack(b, q0, q1, q2, q3);
    fp28_mul(r, a, b);
    return r;
}
__device__ __forceinline__ Fp28 f_mul_v(const Fp28& a, const Fp28& b) { return f_mul_q(a, FP28_AS_QUADS(b)); }
__device__ __forceinline__ Fp28 c_add(const Fp28& a, const Fp28& b) { Fp28 r; f_add(r, a, b); return r; }
__device__ __forceinline__ Fp28 c_sub(const Fp28& a, const Fp28& b) { Fp28 r; f_sub(r, a, b); return r; }
__device__ __forceinline__ Fp28 c_dbl(const Fp28& a) { Fp28 r; f_add(r, a, a); return r; }
__device__ __forceinline__ Fp28 c_neg(const Fp28& a) {
    Fp28 r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = -a.l[i];
    return r;
}

struct G2C { Fp28 x, y, z; };   // this lane's coefficient of the three Jacobian coordinates

// two lanes per pair: write the 68-step line stream of pair `pid` (check = pid / k, j = pid % k);
// lane c writes the records of Fp2 coefficient c.  The k pairs are pairs j0 .. j0+k-1 of the check's k_in
// input pairs (k_in > k when a check is processed in groups of at most eight pairs).
constexpr int PREP_WAVES = 2;   // measured: 256 VGPRs (2 waves/SIMD) 6.6 ms, 168 -> 9.3 ms, 128 -> 11.4 ms per 2^17 pairs (spill traffic)
// y^2 == x^3 + 4 xi for the lane pair's Fp2 point (x, y)?  Inline products (c_mul's arithmetic): a call ahead of the asm loop of
// k_prep_lines costs the loop its registers (compiled that way: 192 B of scratch per lane).  Under full EXEC (DPP partner exchange).
__device__ __forceinline__ Fp28 pair_mul_inline(const Fp28& a, const Fp28& b, int c) {
    Fp28 ao, bo, r;
    swap_pair(ao, a);
    swap_pair(bo, b);
    int32_t x1[NL], x2[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) {
        x1[i] = c ? ao.l[i] : a.l[i];
        x2[i] = c ? a.l[i] : -ao.l[i];
    }
    Acc acc;
    acc_zero(acc);
    acc_mul(acc, x1, b.l);
    acc_mul(acc, x2, bo.l);
    acc_reduce(r.l, acc);
    return r;
}
__device__ __forceinline__ bool on_twist_pair(const Fp28& x, const Fp28& y, int c) {
    Fp28 b4;
    f_set(b4, K28_ONE);
    b4 = c_dbl(c_dbl(b4));                     // 4 xi = 4 + 4 u: 4 in both coefficients
    const Fp28 d = c_sub(c_sub(pair_mul_inline(y, y, c), pair_mul_inline(pair_mul_inline(x, x, c), x, c)), b4);
    Acc acc;
    acc_zero(acc);
#pragma unroll
    for (int i = 0; i < NL; i++) acc.c[i] = d.l[i];
    int32_t t[NL];
    acc_reduce(t, acc);
    uint32_t f[NL];
    canon28(f, t);
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) o |= f[i];
    const int z = o == 0 ? 1 : 0;
    return z && __builtin_amdgcn_update_dpp(0, z, 0xB1, 0xf, 0xf, false);
}

// PREP_CLN: Costello-Lange-Naehrig steps in homogeneous projective coordinates with freely scaled lines (tools/prepasm.py), for the
// fused pairing paths only - any factor of the Miller value that lies in Fp2 dies in the final exponentiation; PREP_JAC: the
// upstream-shaped Jacobian steps of ePrint 2010/354 Alg. 26 / 27 (zkp_multi_miller_loop_batch exposes that Miller value).
// The CLN doubling has b' = 4 xi built in, so on a G2 point off the twist it computes another function: a PREP_CLN wavefront with a
// live pair (no infinity) off the twist stores nothing, and PREP_JAC_OFF_TWIST - launched after it on the same grid - runs exactly
// those wavefronts on the Jacobian steps (same records, same order; on the twist the two line shapes differ by Fp2 factors only).
// Valid inputs never leave the CLN steps; the test costs three Fp2 products per pair.  One body, three kernels (below).
enum { PREP_JAC = 0, PREP_CLN = 1, PREP_JAC_OFF_TWIST = 2 };
template <int MODE>
__device__ __forceinline__ void prep_lines(const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, uint32_t n_pairs_in,
                                           uint32_t k, uint32_t k_in, uint32_t j0, uint32_t nc_in, int4* lines, NDev nd) {
    // nc_in checks of k pairs each (n_pairs_in = nc_in * k); with a device-resident count the launch covers the checks that exist, and
    // their number is the stride of the line records (k_coop computes the same)
    const uint32_t nc = eff_n(nc_in, nd);
    const uint32_t n_pairs = nd.cnt ? nc * k : n_pairs_in;
    if (blockIdx.x * 32u >= n_pairs) return;
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = (int)(tid & 1);
    uint32_t pid = tid >> 1;
    const bool live_lane = pid < n_pairs;
    if (!live_lane) pid = n_pairs - 1;   // keep both lanes of a pair (and the DPP swaps) well defined
    const uint32_t check = pid / k, j = pid - check * k;
    const size_t src = (size_t)check * k_in + j0 + j;
    const bool dead = (inf1 && inf1[src]) || (inf2 && inf2[src]);
    auto rec = [&](uint32_t step, uint32_t e) -> int4* { return lines + ((((size_t)step * k + j) * 6 + e) * nc + check) * 4; };
    // P = (px, py) and Q = (qx, qy) are needed once per step / five times per loop: parked in LDS (limb quad q of
    // value v at [(v * 4 + q) * 64 + lane], conflict-free) instead of occupying 56 VGPRs across every call
    extern __shared__ int4 park[];           // 4 values x 4 quads x 64 lanes, at LDS address 0 (the asm step reads xP, yP by lane number)
    const int lane = threadIdx.x;
    enum { PX = 0, PY = 1, QX = 2, QY = 3 };
    auto park_st = [&](int v, const Fp28& x) {
        park[(v * 4 + 0) * 64 + lane] = make_int4(x.l[0], x.l[1], x.l[2], x.l[3]);
        park[(v * 4 + 1) * 64 + lane] = make_int4(x.l[4], x.l[5], x.l[6], x.l[7]);
        park[(v * 4 + 2) * 64 + lane] = make_int4(x.l[8], x.l[9], x.l[10], x.l[11]);
        park[(v * 4 + 3) * 64 + lane] = make_int4(x.l[12], x.l[13], 0, 0);
    };
    G2C r;
    {
        Fp28 t;
        fp28_from_wire(t, g1 + 12 * src);
        park_st(PX, t);
        fp28_from_wire(t, g1 + 12 * src + 6);
        park_st(PY, t);
        fp28_from_wire(r.x, g2 + 24 * src + 6 * c);
        park_st(QX, r.x);
        fp28_from_wire(r.y, g2 + 24 * src + 12 + 6 * c);
        park_st(QY, r.y);
    }
    constexpr bool CLN = MODE == PREP_CLN;
    if (MODE != PREP_JAC) {        // wave-uniform: each wavefront is run by exactly one of the two fused launches
        const bool off_wave = __ballot(live_lane && !dead && !on_twist_pair(r.x, r.y, c)) != 0;
        if (off_wave != (MODE == PREP_JAC_OFF_TWIST)) return;
    }
    if (c == 0) f_set(r.z, K28_ONE); else f_zero(r.z);
    if (CLN) r.z = c_dbl(r.z);    // W = 2 Z
    uint32_t step = 0;
    // stream order (c2, c1 * xP, c0 * yP) = the (c0, c1, c4) operands of mul_by_014; a pair with an infinity streams
    // the neutral line (1, 0, 0)
    // the asm steps store the lines of live pairs without an infinity only; a pair with an infinity streams the neutral line
    // (1, 0, 0) at every step - written here, ahead of the loop, so that none of this is alive across the blocks
    if (live_lane && dead) {
        Fp28 o;
        for (uint32_t st = 0; st < (uint32_t)NLINES; st++) {
            for (uint32_t e = 0; e < 6; e += 2) {
                if (e == 0 && c == 0) f_set(o, K28_ONE); else f_zero(o);
                rec_store(rec(st, e + c), o);
            }
        }
    }
    // bits of |x| below its leading one: a doubling step each, an addition step after it where the bit is set
    // (the lowest bit is clear: the loop ends with the final doubling) -> 63 + 5 = 68 line records
    const uint64_t xs = 0xd201000000010000ULL;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        // the step's three line records leave from inside the block (lanes of live pairs without an infinity); a pair with an
        // infinity got the neutral lines ahead of the loop
#define ZKP_PREP_STEP_ASM(BLOCK)                                                                                                          \
        do {                                                                                                                              \
            constexpr uint32_t PL[NL] = {ZKP28_P_LIMBS};                                                                                  \
            const unsigned long long smask = __ballot(live_lane && !dead);                                                                 \
            const uint64_t sb_ = (uint64_t)(uintptr_t)lines + (uint64_t)step * k * 6 * nc * 64;   /* wave-uniform: made scalar by hand */ \
            const char* const sbase = (const char*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(sb_ >> 32)) << 32) |  \
                                                    (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)sb_));                  \
            const uint32_t voff = (uint32_t)(((size_t)j * 6 + c) * nc + check) * 64u;                                                     \
            asm volatile(BLOCK                                                                                                            \
                         : ZKP_PREP_DBL_IO(r.x.l, r.y.l, r.z.l)                                                                           \
                         : [estride] "s"(2u * nc * 64u), [voff] "v"(voff), [smask] "s"(smask), [base] "s"(sbase),                         \
                           [p0] "s"(PL[0]), [p1] "s"(PL[1]), [p2] "s"(PL[2]), [p3] "s"(PL[3]), [p4] "s"(PL[4]), [p5] "s"(PL[5]),         \
                           [p6] "s"(PL[6]), [p7] "s"(PL[7]), [p8] "s"(PL[8]), [p9] "s"(PL[9]), [p10] "s"(PL[10]), [p11] "s"(PL[11]),     \
                           [p12] "s"(PL[12]), [p13] "s"(PL[13]), [pinv] "s"(ZKP28_PINV)                                                   \
                         : ZKP_PREP_DBL_CLOBBERS);                                                                                        \
        } while (0)
        static_assert(NL == 14, "the generated blocks are for 14 limbs");
        // <false>: the Jacobian doubling with the upstream-shaped lines (round 4: generate_jac, 18 Karatsuba blocks + 12 reductions)
        if (CLN) ZKP_PREP_STEP_ASM(ZKP_PREP_DBL_ASM); else ZKP_PREP_STEP_ASM(ZKP_PREP_JAC_DBL_ASM);
        step++;
        if ((xs >> b) & 1) {
            if (CLN) ZKP_PREP_STEP_ASM(ZKP_PREP_ADD_ASM); else ZKP_PREP_STEP_ASM(ZKP_PREP_JAC_ADD_ASM);
            step++;
        }
    }
}
// k_prep_lines<true>: the fused paths' CLN steps; k_prep_lines<false>: the Jacobian steps of zkp_multi_miller_loop_batch;
// k_prep_lines_off_twist: the fused paths' wavefronts with a G2 point off the twist, on the Jacobian steps
template <bool CLN>
__global__ void __launch_bounds__(64, PREP_WAVES) k_prep_lines(const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2,
                                                       uint32_t n_pairs_in, uint32_t k, uint32_t k_in, uint32_t j0, uint32_t nc_in, int4* lines, NDev nd) {
    prep_lines<CLN ? PREP_CLN : PREP_JAC>(g1, g2, inf1, inf2, n_pairs_in, k, k_in, j0, nc_in, lines, nd);
}
__global__ void __launch_bounds__(64, PREP_WAVES) k_prep_lines_off_twist(const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1,
                                                                 const uint8_t* inf2, uint32_t n_pairs_in, uint32_t k, uint32_t k_in, uint32_t j0,
                                                                 uint32_t nc_in, int4* lines, NDev nd) {
    prep_lines<PREP_JAC_OFF_TWIST>(g1, g2, inf1, inf2, n_pairs_in, k, k_in, j0, nc_in, lines, nd);
}

// =============================================================================== validity checks on the 28-bit core
// G1Affine::is_valid / G2Affine::is_valid (reference src/g1.rs:49-62, src/g2.rs:57-69) with Jacobian arithmetic and
// no inversion.  Zero tests canonicalise (one reduction); every exceptional case of the group law is handled so
// that the status agrees with the affine reference semantics on EVERY input (small-order points included).
__device__ __forceinline__ bool f_is_zero(const Fp28& a) {
    Acc acc;
    acc_zero(acc);
#pragma unroll
    for (int i = 0; i < NL; i++) acc.c[i] = a.l[i];
    int32_t x[NL];
    acc_reduce(x, acc);
    uint32_t f[NL];
    canon28(f, x);
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) o |= f[i];
    return o == 0;
}
__device__ __forceinline__ Fp28 f_const(const int32_t* k) { Fp28 r; f_set(r, k); return r; }
__device__ __forceinline__ Fp28 f_vred(Fp28 a) { vred(a.l); return a; }

// ---- generic Jacobian arithmetic over an "element" E with by-value ops supplied by the policy F
//      (F1: Fp, one lane per point; F2: Fp2 spread over a lane pair)
// the affine input point of a validity check, parked in LDS (limb quad q of value v at [(v * 4 + q) * 64 + lane])
__device__ __forceinline__ void valid_park(int4* park, int lane, int v, const Fp28& x) {
    park[(v * 4 + 0) * 64 + lane] = make_int4(x.l[0], x.l[1], x.l[2], x.l[3]);
    park[(v * 4 + 1) * 64 + lane] = make_int4(x.l[4], x.l[5], x.l[6], x.l[7]);
    park[(v * 4 + 2) * 64 + lane] = make_int4(x.l[8], x.l[9], x.l[10], x.l[11]);
    park[(v * 4 + 3) * 64 + lane] = make_int4(x.l[12], x.l[13], 0, 0);
}
__device__ __forceinline__ Fp28 valid_unpark(const int4* park, int lane, int v) {
    asm volatile("" ::: "memory");   // keep the load at its use
    const int4 v0 = park[(v * 4 + 0) * 64 + lane], v1 = park[(v * 4 + 1) * 64 + lane], v2 = park[(v * 4 + 2) * 64 + lane],
               v3 = park[(v * 4 + 3) * 64 + lane];
    Fp28 x;
    x.l[0] = v0.x; x.l[1] = v0.y; x.l[2] = v0.z; x.l[3] = v0.w; x.l[4] = v1.x; x.l[5] = v1.y; x.l[6] = v1.z; x.l[7] = v1.w;
    x.l[8] = v2.x; x.l[9] = v2.y; x.l[10] = v2.z; x.l[11] = v2.w; x.l[12] = v3.x; x.l[13] = v3.y;
    return x;
}
struct F1 {
    int c;
    __device__ Fp28 sqr(const Fp28& a) const { return f_mul_v(a, a); }
    __device__ Fp28 mul(const Fp28& a, const Fp28& b) const { return f_mul_v(a, b); }
    __device__ bool is_zero(const Fp28& a) const { return f_is_zero(a); }
    __device__ Fp28 one() const { return f_const(K28_ONE); }
};
struct F2 {
    int c;   // which Fp2 coefficient this lane holds
    __device__ Fp28 sqr(const Fp28& a) const { return c_sqr(a, c); }
    __device__ Fp28 mul(const Fp28& a, const Fp28& b) const { return c_mul(a, b, c); }
    __device__ bool is_zero(const Fp28& a) const {
        const int z = f_is_zero(a) ? 1 : 0;
        const int zo = __builtin_amdgcn_update_dpp(0, z, 0xB1, 0xf, 0xf, false);
        return z && zo;
    }
    __device__ Fp28 one() const { Fp28 r; if (c == 0) f_set(r, K28_ONE); else f_zero(r); return r; }
};
struct JacP { Fp28 x, y, z; };   // z == 0 <=> infinity

// a = 0 doubling (dbl-2009-l).  Infinity and y = 0 need no special case: Z3 = 2 Y Z vanishes.
// Ordered for few live values (at most five 14-register values across any call: the by-value routines keep the caller's
// values in the ~108 callee-saved VGPRs, anything beyond that is spilled around every call).
template <class F>
__device__ __forceinline__ void jac_dbl(const F& f, JacP& p) {
    Fp28 B = f.sqr(p.y);
    Fp28 Z3 = c_dbl(f.mul(p.y, p.z));
    Fp28 A = f.sqr(p.x);
    Fp28 t = f.sqr(c_add(p.x, B));
    Fp28 C = f.sqr(B);
    Fp28 D = c_dbl(c_sub(c_sub(t, A), C));
    Fp28 E = c_add(c_add(A, A), A);
    Fp28 X3 = c_sub(c_sub(f.sqr(E), D), D);
    Fp28 Y3 = c_sub(f.mul(E, c_sub(D, X3)), c_dbl(c_dbl(c_dbl(C))));
    p.x = f_vred(X3); p.y = f_vred(Y3); p.z = f_vred(Z3);
}
// mixed addition p += (qx, qy) (madd-2007-bl) with every exceptional case; the affine point comes through a loader (it is
// parked in LDS: held in registers it would be ten live values across every doubling of the scalar multiplication)
template <class F, class Q>
__device__ __forceinline__ void jac_madd(const F& f, JacP& p, Q&& ldq) {
    if (f.is_zero(p.z)) { p.x = ldq(0); p.y = ldq(1); p.z = f.one(); return; }
    Fp28 Z1Z1 = f.sqr(p.z);
    Fp28 H = c_sub(f.mul(ldq(0), Z1Z1), p.x);
    Fp28 rr = c_sub(f.mul(f.mul(ldq(1), p.z), Z1Z1), p.y);
    if (f.is_zero(H)) {
        if (f.is_zero(rr)) { p.x = ldq(0); p.y = ldq(1); p.z = f.one(); jac_dbl(f, p); return; }
        f_zero(p.z);   // P + (-P)
        return;
    }
    Fp28 HH = f.sqr(H);
    Fp28 Z3 = c_sub(c_sub(f.sqr(c_add(p.z, H)), Z1Z1), HH);
    rr = c_dbl(rr);
    Fp28 I = c_dbl(c_dbl(HH));
    Fp28 V = f.mul(p.x, I);
    Fp28 J = f.mul(H, I);
    Fp28 X3 = c_sub(c_sub(c_sub(f.sqr(rr), J), V), V);
    Fp28 Y3 = c_sub(f.mul(rr, c_sub(V, X3)), c_dbl(f.mul(p.y, J)));
    p.x = f_vred(X3); p.y = f_vred(Y3); p.z = f_vred(Z3);
}
// p = [k] Q, Q behind the loader, k given as nwords 64-bit words, MSB first
template <class F, class Q>
__device__ __forceinline__ void jac_mul(const F& f, JacP& p, Q&& ldq, const uint64_t* k, int nwords) {
    p.x = f.one(); p.y = f.one(); f_zero(p.z);
#pragma unroll 1
    for (int w = nwords - 1; w >= 0; w--) {
        const uint64_t e = k[w];
#pragma unroll 1
        for (int b = 63; b >= 0; b--) {
            jac_dbl(f, p);
            if ((e >> b) & 1) jac_madd(f, p, ldq);
        }
    }
}
// Jacobian p == affine (qx, qy) ?  (infinity never equals a finite point)
template <class F>
__device__ __forceinline__ bool jac_eq_affine(const F& f, const JacP& p, const Fp28& qx, const Fp28& qy) {
    if (f.is_zero(p.z)) return false;
    Fp28 z2 = f.sqr(p.z);
    Fp28 z3 = f.mul(z2, p.z);
    const bool ex = f.is_zero(c_sub(f.mul(qx, z2), p.x));
    const bool ey = f.is_zero(c_sub(f.mul(qy, z3), p.y));
    return ex && ey;
}

// one lane per point: 0 valid / 1 not on curve / 2 not torsion free  (-[X^2]P == (beta x, y), src/g1.rs:111-115)
// redo_only: the asm kernel ran first and left VALID_REDO where its chain met an exceptional case of the group law (infinity,
// P + P, P - P, order two: points outside the prime-order subgroup only) - this kernel, which handles every case, redoes those
constexpr uint8_t VALID_REDO = 0xff;
__global__ void __launch_bounds__(64, 2) k_g1_valid28(const uint64_t* g1, const uint8_t* inf, uint32_t n, uint8_t* status, int redo_only) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    if (redo_only && status[i] != VALID_REDO) return;
    if (inf && inf[i]) { status[i] = 0; return; }
    F1 f{0};
    Fp28 x, y;
    fp28_from_wire(x, g1 + 12 * (size_t)i);
    fp28_from_wire(y, g1 + 12 * (size_t)i + 6);
    Fp28 lhs = f.sqr(y);
    Fp28 rhs = c_add(f.mul(f.sqr(x), x), f_const(K28_B));
    if (!f.is_zero(c_sub(lhs, rhs))) { status[i] = 1; return; }
    const uint64_t x2[2] = {0x0000000100000000ULL, 0xac45a4010001a402ULL};   // X^2, X = 0xd201000000010000
    __shared__ int4 park[2 * 4 * 64];
    const int lane = threadIdx.x;
    valid_park(park, lane, 0, x);
    valid_park(park, lane, 1, y);
    auto ldq = [&](int v) -> Fp28 { return valid_unpark(park, lane, v); };
    JacP p;
    jac_mul(f, p, ldq, x2, 2);
    Fp28 bx = f.mul(ldq(0), f_const(K28_BETA));
    status[i] = jac_eq_affine(f, p, bx, c_neg(ldq(1))) ? 0 : 2;
}

// two lanes per point: psi(P) == -[X]P  (src/g2.rs:166-170)
__global__ void __launch_bounds__(64, 2) k_g2_valid28(const uint64_t* g2, const uint8_t* inf, uint32_t n, uint8_t* status, int redo_only) {
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = (int)(tid & 1);
    uint32_t i = tid >> 1;
    const bool live = i < n;
    if (!live) i = n - 1;
    if (redo_only && !__any(live && status[i] == VALID_REDO)) return;      // wave-uniform: both lanes of a pair stay together
    const bool keep = redo_only && status[i] != VALID_REDO;
    const bool is_inf = inf && inf[i];
    __shared__ int4 park[2 * 4 * 64];
    const int lane = threadIdx.x;
    F2 f{c};
    Fp28 x, y;
    fp28_from_wire(x, g2 + 24 * (size_t)i + 6 * c);
    fp28_from_wire(y, g2 + 24 * (size_t)i + 12 + 6 * c);
    uint8_t st;
    Fp28 lhs = f.sqr(y);
    Fp28 rhs = c_add(f.mul(f.sqr(x), x), f_const(K28_B));     // b' = 4 (1 + u): both coefficients are 4
    if (!f.is_zero(c_sub(lhs, rhs))) {
        st = 1;
    } else {
        const uint64_t xs[1] = {0xd201000000010000ULL};
        valid_park(park, lane, 0, x);
        valid_park(park, lane, 1, y);
        auto ldq = [&](int v) -> Fp28 { return valid_unpark(park, lane, v); };
        JacP p;
        jac_mul(f, p, ldq, xs, 1);
        x = ldq(0); y = ldq(1);
        // psi(P) = (conj(x) PSI_X, conj(y) PSI_Y); compare [X]P with (psi_x, -psi_y)
        Fp28 cx = c ? c_neg(x) : x, cy = c ? c_neg(y) : y;
        Fp28 kx = f_const(c ? K28_PSI_X_1 : K28_PSI_X_0), ky = f_const(c ? K28_PSI_Y_1 : K28_PSI_Y_0);
        Fp28 px = f.mul(cx, kx), py = f.mul(cy, ky);
        st = jac_eq_affine(f, p, px, c_neg(py)) ? 0 : 2;
    }
    if (live && c == 0 && !keep) status[i] = is_inf ? 0 : st;
}

// ---- the same two checks with the chain's steps as asm blocks (tools/validasm.py).  No exceptional case of the group law is
// handled in the steps: each of them sends Z to 0, Z = 0 is absorbing, and a chain that ends with Z = 0 mod p is handed to
// the generic kernel above (status VALID_REDO; launched behind this one with redo_only).  A point of the prime-order subgroup
// never takes that route: the chains' scalars (x^2, |x|) are below r.
// one lane per point, three waves per SIMD: -[x^2] P == (beta x, y)  (src/g1.rs:111-115)
__global__ void __launch_bounds__(64, 3) k_g1_valid_fast(const uint64_t* g1, const uint8_t* inf, uint32_t n, uint8_t* status) {
    extern __shared__ int4 park[];          // slots 0, 1: the affine point, 2: the addition's parked value; at LDS address 0
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * 64 + lane;
    const bool live = i < n;
    if (!live) i = n - 1;
    const bool is_inf = inf && inf[i];
    bool on;
    int32_t X[NL], Y[NL], Z[NL];
    {
        Fp28 x, y;
        fp28_from_wire(x, g1 + 12 * (size_t)i);
        fp28_from_wire(y, g1 + 12 * (size_t)i + 6);
        Fp28 lhs, t, rhs;
        fp28_mul(lhs, y, y);
        fp28_mul(t, x, x);
        fp28_mul(rhs, t, x);
        on = f_is_zero(c_sub(lhs, c_add(rhs, f_const(K28_B))));
        valid_park(park, lane, 0, x);
        valid_park(park, lane, 1, y);
#pragma unroll
        for (int k = 0; k < NL; k++) { X[k] = x.l[k]; Y[k] = y.l[k]; Z[k] = K28_ONE[k]; }
    }
    if (!__any(on && !is_inf)) {            // wave-uniform: nothing to multiply
        if (live) status[i] = is_inf ? 0 : 1;
        return;
    }
    // the blocks own v6..v167 of the 168 registers of three waves per SIMD: what the epilogue needs of the lane is ONE packed
    // register here and is re-derived from an opaque copy of the lane number behind the loop
    int flags = (on ? 1 : 0) | (is_inf ? 2 : 0);
    static_assert(NL == 14, "the generated blocks are for 14 limbs");
#define ZKP_G1_STEP(BLOCK)                                                                                                               \
    do {                                                                                                                                 \
        constexpr uint32_t PL[NL] = {ZKP28_P_LIMBS};                                                                                     \
        asm volatile(BLOCK                                                                                                               \
                     : ZKP_G1_STEP_IO(X, Y, Z)                                                                                           \
                     : [p0] "s"(PL[0]), [p1] "s"(PL[1]), [p2] "s"(PL[2]), [p3] "s"(PL[3]), [p4] "s"(PL[4]), [p5] "s"(PL[5]),            \
                       [p6] "s"(PL[6]), [p7] "s"(PL[7]), [p8] "s"(PL[8]), [p9] "s"(PL[9]), [p10] "s"(PL[10]), [p11] "s"(PL[11]),        \
                       [p12] "s"(PL[12]), [p13] "s"(PL[13]), [pinv] "s"(ZKP28_PINV)                                                      \
                     : ZKP_G1_STEP_CLOBBERS);                                                                                            \
    } while (0)
    // X^2 = 0xac45a4010001a402_0000000100000000 (X = 0xd201000000010000): the accumulator starts at P (the leading one), then
    // one doubling per remaining bit and an addition where the bit is set
    const uint64_t hi = 0xac45a4010001a402ULL, lo = 0x0000000100000000ULL;
#pragma unroll 1
    for (int b = 126; b >= 0; b--) {
        ZKP_G1_STEP(ZKP_G1_DBL_ASM);
        if (((b >= 64 ? hi >> (b - 64) : lo >> b) & 1) != 0) ZKP_G1_STEP(ZKP_G1_MADD_ASM);
    }
    int l_ = threadIdx.x;
    asm volatile("" : "+v"(l_), "+v"(flags));
    Fp28 px, py, pz;
#pragma unroll
    for (int k = 0; k < NL; k++) { px.l[k] = X[k]; py.l[k] = Y[k]; pz.l[k] = Z[k]; }
    uint8_t st;
    if (f_is_zero(pz)) {
        st = VALID_REDO;
    } else {
        Fp28 z2, z3, bx, t;
        fp28_mul(z2, pz, pz);
        fp28_mul(z3, z2, pz);
        fp28_mul(bx, valid_unpark(park, l_, 0), f_const(K28_BETA));
        fp28_mul(t, bx, z2);
        const bool ex = f_is_zero(c_sub(t, px));
        fp28_mul(t, c_neg(valid_unpark(park, l_, 1)), z3);
        const bool ey = f_is_zero(c_sub(t, py));
        st = ex && ey ? 0 : 2;
    }
    const uint32_t i_ = blockIdx.x * 64 + (uint32_t)l_;
    if (i_ < n) status[i_] = (flags & 2) ? 0 : ((flags & 1) ? st : 1);
}

// two lanes per point: psi(P) == -[X] P  (src/g2.rs:166-170)
__global__ void __launch_bounds__(64, 2) k_g2_valid_fast(const uint64_t* g2, const uint8_t* inf, uint32_t n, uint8_t* status) {
    extern __shared__ int4 park[];          // values 0, 1: this lane's coefficient of the affine point; at LDS address 0
    const int lane = threadIdx.x;
    const uint32_t tid = blockIdx.x * 64 + lane;
    const int c = (int)(tid & 1);
    uint32_t i = tid >> 1;
    const bool live = i < n;
    if (!live) i = n - 1;
    const bool is_inf = inf && inf[i];
    F2 f{c};
    bool on;
    G2C r;
    {
        Fp28 x, y;
        fp28_from_wire(x, g2 + 24 * (size_t)i + 6 * c);
        fp28_from_wire(y, g2 + 24 * (size_t)i + 12 + 6 * c);
        Fp28 lhs = f.sqr(y);
        Fp28 rhs = c_add(f.mul(f.sqr(x), x), f_const(K28_B));     // b' = 4 (1 + u): both coefficients are 4
        on = f.is_zero(c_sub(lhs, rhs));
        valid_park(park, lane, 0, x);
        valid_park(park, lane, 1, y);
        r.x = x;
        r.y = y;
        r.z = f.one();
    }
    if (!__any(on && !is_inf)) {
        if (live && c == 0) status[i] = is_inf ? 0 : 1;
        return;
    }
#define ZKP_G2_STEP(BLOCK)                                                                                                               \
    do {                                                                                                                                 \
        constexpr uint32_t PL[NL] = {ZKP28_P_LIMBS};                                                                                     \
        asm volatile(BLOCK                                                                                                               \
                     : ZKP_G2_STEP_IO(r.x.l, r.y.l, r.z.l)                                                                               \
                     : [p0] "s"(PL[0]), [p1] "s"(PL[1]), [p2] "s"(PL[2]), [p3] "s"(PL[3]), [p4] "s"(PL[4]), [p5] "s"(PL[5]),            \
                       [p6] "s"(PL[6]), [p7] "s"(PL[7]), [p8] "s"(PL[8]), [p9] "s"(PL[9]), [p10] "s"(PL[10]), [p11] "s"(PL[11]),        \
                       [p12] "s"(PL[12]), [p13] "s"(PL[13]), [pinv] "s"(ZKP28_PINV)                                                      \
                     : ZKP_G2_STEP_CLOBBERS);                                                                                            \
    } while (0)
    const uint64_t xs = 0xd201000000010000ULL;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        ZKP_G2_STEP(ZKP_G2_DBL_ASM);
        if ((xs >> b) & 1) ZKP_G2_STEP(ZKP_G2_MADD_ASM);
    }
    uint8_t st;
    JacP p{r.x, r.y, r.z};
    if (f.is_zero(p.z)) {
        st = VALID_REDO;
    } else {
        Fp28 x = valid_unpark(park, lane, 0), y = valid_unpark(park, lane, 1);
        // psi(P) = (conj(x) PSI_X, conj(y) PSI_Y); compare [X] P with (psi_x, -psi_y)
        Fp28 cx = c ? c_neg(x) : x, cy = c ? c_neg(y) : y;
        Fp28 kx = f_const(c ? K28_PSI_X_1 : K28_PSI_X_0), ky = f_const(c ? K28_PSI_Y_1 : K28_PSI_Y_0);
        Fp28 qx = f.mul(cx, kx), qy = f.mul(cy, ky);
        st = jac_eq_affine(f, p, qx, c_neg(qy)) ? 0 : 2;
    }
    if (live && c == 0) status[i] = is_inf ? 0 : (on ? st : 1);
}

// the same check at THREE waves per SIMD (tools/validasm.py g2_dbl3 / g2_madd3): five register blocks + the Karatsuba product set =
// 168 VGPRs.  Between steps only Y is in registers; X and Z live in LDS slots 0 and 1 (slot 2 parks a value inside the addition), the
// affine point's limbs - needed by the five additions - in `qs`: quad q of value v (0: x, 1: y) of global lane t at
// qs[(v * 4 + q) * lanes + t].
__global__ void __launch_bounds__(64, 3) k_g2_valid_fast3(const uint64_t* g2, const uint8_t* inf, uint32_t n, uint8_t* status, int4* qs) {
    extern __shared__ int4 park[];
    const int lane = threadIdx.x;
    const uint32_t tid = blockIdx.x * 64 + lane;
    const uint32_t lanes = gridDim.x * 64;
    const int c = (int)(tid & 1);
    uint32_t i = tid >> 1;
    if (i >= n) i = n - 1;
    const bool is_inf = inf && inf[i];
    bool on;
    int32_t Y[NL];
    {
        F2 f{c};
        Fp28 x, y;
        fp28_from_wire(x, g2 + 24 * (size_t)i + 6 * c);
        fp28_from_wire(y, g2 + 24 * (size_t)i + 12 + 6 * c);
        Fp28 lhs = f.sqr(y);
        Fp28 rhs = c_add(f.mul(f.sqr(x), x), f_const(K28_B));
        on = f.is_zero(c_sub(lhs, rhs));
        valid_park(park, lane, 0, x);
        valid_park(park, lane, 1, f.one());
        const Fp28* v[2] = {&x, &y};
#pragma unroll
        for (int k = 0; k < 2; k++) {
            qs[(size_t)(k * 4 + 0) * lanes + tid] = make_int4(v[k]->l[0], v[k]->l[1], v[k]->l[2], v[k]->l[3]);
            qs[(size_t)(k * 4 + 1) * lanes + tid] = make_int4(v[k]->l[4], v[k]->l[5], v[k]->l[6], v[k]->l[7]);
            qs[(size_t)(k * 4 + 2) * lanes + tid] = make_int4(v[k]->l[8], v[k]->l[9], v[k]->l[10], v[k]->l[11]);
            qs[(size_t)(k * 4 + 3) * lanes + tid] = make_int4(v[k]->l[12], v[k]->l[13], 0, 0);
        }
#pragma unroll
        for (int k = 0; k < NL; k++) Y[k] = y.l[k];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the lane reads its own scratch records back inside the additions
    if (!__any(on && !is_inf)) {
        if (tid < 2 * n && c == 0) status[i] = is_inf ? 0 : 1;
        return;
    }
    int flags = (on ? 1 : 0) | (is_inf ? 2 : 0);
    const uint32_t qoff = tid * 16u, qstride = lanes * 16u;
    const uint32_t qlo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)qs);
    const uint32_t qhi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)((uintptr_t)qs >> 32));
#define ZKP_G2W3_STEP(BLOCK)                                                                                                             \
    do {                                                                                                                                 \
        constexpr uint32_t PL[NL] = {ZKP28_P_LIMBS};                                                                                     \
        asm volatile(BLOCK                                                                                                               \
                     : ZKP_G2W3_STEP_IO(Y)                                                                                               \
                     : [qoff] "v"(qoff), [qstride] "s"(qstride), [qlo] "s"(qlo), [qhi] "s"(qhi),                                         \
                       [p0] "s"(PL[0]), [p1] "s"(PL[1]), [p2] "s"(PL[2]), [p3] "s"(PL[3]), [p4] "s"(PL[4]), [p5] "s"(PL[5]),            \
                       [p6] "s"(PL[6]), [p7] "s"(PL[7]), [p8] "s"(PL[8]), [p9] "s"(PL[9]), [p10] "s"(PL[10]), [p11] "s"(PL[11]),        \
                       [p12] "s"(PL[12]), [p13] "s"(PL[13]), [pinv] "s"(ZKP28_PINV)                                                      \
                     : ZKP_G2W3_STEP_CLOBBERS);                                                                                          \
    } while (0)
    const uint64_t xs = 0xd201000000010000ULL;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        ZKP_G2W3_STEP(ZKP_G2W3_DBL_ASM);
        if ((xs >> b) & 1) ZKP_G2W3_STEP(ZKP_G2W3_MADD_ASM);
    }
    int l_ = threadIdx.x;
    asm volatile("" : "+v"(l_), "+v"(flags));
    const uint32_t t_ = blockIdx.x * 64 + (uint32_t)l_;
    const int c_ = (int)(t_ & 1);
    uint32_t i_ = t_ >> 1;
    const bool live_ = i_ < n;
    if (!live_) i_ = n - 1;
    F2 f{c_};
    JacP p;
    p.x = valid_unpark(park, l_, 0);
    p.z = valid_unpark(park, l_, 1);
#pragma unroll
    for (int k = 0; k < NL; k++) p.y.l[k] = Y[k];
    uint8_t st;
    if (f.is_zero(p.z)) {
        st = VALID_REDO;
    } else {
        Fp28 x, y;
        fp28_from_wire(x, g2 + 24 * (size_t)i_ + 6 * c_);
        fp28_from_wire(y, g2 + 24 * (size_t)i_ + 12 + 6 * c_);
        Fp28 cx = c_ ? c_neg(x) : x, cy = c_ ? c_neg(y) : y;
        Fp28 kx = f_const(c_ ? K28_PSI_X_1 : K28_PSI_X_0), ky = f_const(c_ ? K28_PSI_Y_1 : K28_PSI_Y_0);
        Fp28 qx = f.mul(cx, kx), qy = f.mul(cy, ky);
        st = jac_eq_affine(f, p, qx, c_neg(qy)) ? 0 : 2;
    }
    if (live_ && c_ == 0) status[i_] = (flags & 2) ? 0 : ((flags & 1) ? st : 1);
}

// a^(p-2) (Fermat; reference src/fp.rs:307-319); a == 0 gives 0.  Kept as the cross-check of f_inv (ZKP_INV_FERMAT).
__device__ __forceinline__ Fp28 f_inv_fermat(const Fp28& a) {
    Fp28 res = f_const(K28_ONE);
#pragma unroll 1
    for (int w = NL - 1; w >= 0; w--) {
        const uint32_t e = (uint32_t)K28_P[w] - (w == 0 ? 2u : 0u);
#pragma unroll 1
        for (int b = W - 1; b >= 0; b--) {
            fp28_mul(res, res, res);
            if ((e >> b) & 1) fp28_mul(res, res, a);
        }
    }
    return res;
}

// a^-1 by Bernstein-Yang division steps ("safegcd", delta = 1 variant; 0 gives 0): the same value as the reference's
// a^(p-2) (src/fp.rs:307-319) with ~26 k instead of ~240 k instructions on the single-lane critical path of the final
// exponentiation.  f = p, g = a as 13 signed limbs of 30 bits; 37 batches of 30 division steps (1110 >= the proven
// bound (49 * 381 + 57) / 17 = 1101 for 381-bit inputs); each batch runs on the low limbs, yields a 2x2 transition matrix
// (entries < 2^30 in magnitude) and is applied to (f, g) exactly and to (d, e) modulo p, d and e staying in (-2p, p).
// Straight-line code: no lane diverges.  Layout of the arithmetic follows libsecp256k1's modinv32 (public domain
// algorithm description in its safegcd_implementation.md); tools/safegcd_model.py is the limb-exact model it was
// checked against on the CPU.
namespace sg {
constexpr int N = 13;
constexpr int32_t M30 = 0x3fffffff;
__device__ __constant__ const int32_t PL[N] = {ZKP30_P_LIMBS};

// Round 6: the transition matrix is tracked in PACKED 16-bit halves - (u, v) in one register, (q, r) in another - over three runs of ten steps
// (entries <= 2^10), and the three 2 x 2 matrices are multiplied together afterwards (24-bit multiplies; the products wrap mod 2^32 and
// the true entries are <= 2^30).  A conditional negation / masked addition / doubling of BOTH entries of a row is one v_pk_* instruction:
// 19 instead of 24 instructions per step.  The same matrix as thirty plain division steps, hence the same inverse:
// tests/test_gpu_parity.py::test_divstep_inversion_equals_fermat.
typedef short zkp_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void divsteps30(int32_t& eta, uint32_t f, uint32_t g, int32_t& u_, int32_t& v_, int32_t& q_, int32_t& r_) {
    uint32_t e = (uint32_t)eta;
    int32_t U = 1, V = 0, Q = 0, R = 1;                        // the product of the runs so far
#pragma unroll
    for (int run = 0; run < 3; run++) {
        zkp_s2 P = {1, 0}, T = {0, 1};                         // rows (u, v) and (q, r) of this run's matrix
#pragma unroll 5
        for (int i = 0; i < 10; i++) {
            uint32_t c1 = (uint32_t)((int32_t)e >> 31);        // eta < 0  <=>  delta > 0
            const uint32_t c2 = 0u - (g & 1u);
            const uint32_t x = (f ^ c1) - c1;
            const zkp_s2 m1 = __builtin_bit_cast(zkp_s2, c1), m2 = __builtin_bit_cast(zkp_s2, c2);
            const zkp_s2 Y = (P ^ m1) - m1;                    // (-u, -v) where delta > 0
            g += x & c2;
            T += Y & m2;
            c1 &= c2;                                          // delta > 0 and g odd: swap roles
            e = (e ^ c1) - (c1 + 1u);
            f += g & c1;
            P += T & __builtin_bit_cast(zkp_s2, c1);
            g >>= 1;
            P += P;                                            // (u, v) <<= 1
        }
        const int32_t u2 = P.x, v2 = P.y, q2 = T.x, r2 = T.y;
        if (run == 0) {
            U = u2; V = v2; Q = q2; R = r2;
        } else {                                               // M <- M_run * M: entries of M_run <= 2^10, of M <= 2^20: 24-bit operands
            const int32_t nU = __mul24(u2, U) + __mul24(v2, Q), nV = __mul24(u2, V) + __mul24(v2, R);
            const int32_t nQ = __mul24(q2, U) + __mul24(r2, Q), nR = __mul24(q2, V) + __mul24(r2, R);
            U = nU; V = nV; Q = nQ; R = nR;
        }
    }
    eta = (int32_t)e; u_ = U; v_ = V; q_ = Q; r_ = R;
}
// Round 6: the limbs and matrix entries are pinned to 32-bit registers (an empty asm the optimiser cannot see through).  Without it
// LLVM carries a limb as the masked 64-bit carry word it came from and expands every (int64) u * limb into the 64 x 64-bit pattern
// (v_mad_u64_u32 x 2 + v_mul_lo_u32 x 2 + moves: 562 instructions for the two updates of a batch); with 32-bit operands each product
// is ONE v_mad_i64_i32.  k_batch_inv is one lane's dependent chain - the six launches of a pass are what a small or medium batch pays in
// full (profiles/r06: 0.11-0.18 ms each, whatever the batch) - so instructions are time here.
#define ZKP_SG_PIN32(x) asm volatile("" : "+v"(x))
// (f, g) <- (u f + v g, q f + r g) / 2^30, exactly
__device__ __forceinline__ void update_fg(int32_t* f, int32_t* g, int32_t u, int32_t v, int32_t q, int32_t r) {
    ZKP_SG_PIN32(u); ZKP_SG_PIN32(v); ZKP_SG_PIN32(q); ZKP_SG_PIN32(r);
    int64_t cf = (int64_t)u * f[0] + (int64_t)v * g[0];
    int64_t cg = (int64_t)q * f[0] + (int64_t)r * g[0];
    cf >>= 30; cg >>= 30;                                      // the low 30 bits are zero by construction
#pragma unroll
    for (int i = 1; i < N; i++) {
        cf += (int64_t)u * f[i] + (int64_t)v * g[i];
        cg += (int64_t)q * f[i] + (int64_t)r * g[i];
        f[i - 1] = (int32_t)cf & M30; cf >>= 30;
        g[i - 1] = (int32_t)cg & M30; cg >>= 30;
        ZKP_SG_PIN32(f[i - 1]); ZKP_SG_PIN32(g[i - 1]);
    }
    f[N - 1] = (int32_t)cf; g[N - 1] = (int32_t)cg;
    ZKP_SG_PIN32(f[N - 1]); ZKP_SG_PIN32(g[N - 1]);
}
// (d, e) <- (u d + v e, q d + r e) / 2^30 mod p; inputs and outputs in (-2p, p)
__device__ __forceinline__ void update_de(int32_t* d, int32_t* e, int32_t u, int32_t v, int32_t q, int32_t r) {
    ZKP_SG_PIN32(u); ZKP_SG_PIN32(v); ZKP_SG_PIN32(q); ZKP_SG_PIN32(r);
    const int32_t sd = d[N - 1] >> 31, se = e[N - 1] >> 31;
    int32_t md = (u & sd) + (v & se), me = (q & sd) + (r & se);   // add p to a negative d / e first
    int64_t cd = (int64_t)u * d[0] + (int64_t)v * e[0];
    int64_t ce = (int64_t)q * d[0] + (int64_t)r * e[0];
    md -= (int32_t)((ZKP30_PINV * (uint32_t)cd + (uint32_t)md) & (uint32_t)M30);   // multiple of p that clears the low 30 bits
    me -= (int32_t)((ZKP30_PINV * (uint32_t)ce + (uint32_t)me) & (uint32_t)M30);
    ZKP_SG_PIN32(md); ZKP_SG_PIN32(me);
    cd += (int64_t)PL[0] * md; ce += (int64_t)PL[0] * me;
    cd >>= 30; ce >>= 30;
#pragma unroll
    for (int i = 1; i < N; i++) {
        cd += (int64_t)u * d[i] + (int64_t)v * e[i] + (int64_t)PL[i] * md;
        ce += (int64_t)q * d[i] + (int64_t)r * e[i] + (int64_t)PL[i] * me;
        d[i - 1] = (int32_t)cd & M30; cd >>= 30;
        e[i - 1] = (int32_t)ce & M30; ce >>= 30;
        ZKP_SG_PIN32(d[i - 1]); ZKP_SG_PIN32(e[i - 1]);
    }
    d[N - 1] = (int32_t)cd; e[N - 1] = (int32_t)ce;
    ZKP_SG_PIN32(d[N - 1]); ZKP_SG_PIN32(e[N - 1]);
}
// x in (-2p, p), negated when sign < 0, brought to [0, p)
__device__ __forceinline__ void normalize(int32_t* x, int32_t sign) {
    int32_t add = x[N - 1] >> 31;
    const int32_t neg = sign >> 31;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        int32_t t = x[i] + (PL[i] & add);
        t = (t ^ neg) - neg;
        t += c;
        if (i < N - 1) { x[i] = t & M30; c = t >> 30; } else x[i] = t;
    }
    add = x[N - 1] >> 31;
    c = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const int32_t t = x[i] + (PL[i] & add) + c;
        if (i < N - 1) { x[i] = t & M30; c = t >> 30; } else x[i] = t;
    }
}
}  // namespace sg

__device__ __noinline__ Fp28 f_inv(Fp28 a) {
    // canonical value of the stored (Montgomery) representative, repacked from 14 x 28 to 13 x 30 bits.  a * R / R
    // first: the same value, but certainly inside canon28's input range whatever linear combination a came from
    uint32_t c28[NL];
    {
        Fp28 t;
        fp28_mul(t, a, f_const(K28_ONE));
        canon28(c28, t.l);
    }
    int32_t f[sg::N], g[sg::N], d[sg::N], e[sg::N];
#pragma unroll
    for (int i = 0; i < sg::N; i++) {
        const int bit = 30 * i, wd = bit / W, sh = bit % W;
        uint64_t v = (uint64_t)c28[wd] >> sh;
        if (wd + 1 < NL) v |= (uint64_t)c28[wd + 1] << (W - sh);
        if (wd + 2 < NL) v |= (uint64_t)c28[wd + 2] << (2 * W - sh);
        g[i] = (int32_t)(v & (uint64_t)sg::M30);
        f[i] = sg::PL[i];
        d[i] = 0;
        e[i] = i == 0 ? 1 : 0;
    }
    int32_t eta = -1;
#pragma unroll 1
    for (int it = 0; it < 37; it++) {
        int32_t u, v, q, r;
        sg::divsteps30(eta, (uint32_t)f[0], (uint32_t)g[0], u, v, q, r);
        sg::update_de(d, e, u, v, q, r);
        sg::update_fg(f, g, u, v, q, r);
    }
    sg::normalize(d, f[sg::N - 1]);            // f = +-1 (or +-p with d = 0 when a == 0)
    // 13 x 30 -> 14 x 28 bits; the value is (a R)^-1, and (a R)^-1 * R^3 / R = a^-1 R: the Montgomery form of a^-1
    Fp28 w;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const int bit = W * i, wd = bit / 30, sh = bit % 30;
        uint64_t v = (uint64_t)(uint32_t)d[wd] >> sh;
        if (wd + 1 < sg::N) v |= (uint64_t)(uint32_t)d[wd + 1] << (30 - sh);
        w.l[i] = (int32_t)(v & (uint64_t)MASK);
    }
    Fp28 res;
    fp28_mul(res, w, f_const(K28_R3));
    return res;
}

// [k] P for 256-bit scalars, affine in / affine out (&G1Affine * &Fr, reference src/g1.rs:130-153 without its dropped
// bit 0; src/g2.rs:185-208).  One lane per G1 point; two lanes per G2 point.
__global__ void __launch_bounds__(64, 2) k_g1_mul28(const uint64_t* base, size_t stride, const uint64_t* sc, uint32_t n, uint64_t* out, uint8_t* out_inf) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    F1 f{0};
    Fp28 x, y;
    fp28_from_wire(x, base + stride * i);
    fp28_from_wire(y, base + stride * i + 6);
    const uint64_t k[4] = {sc[4 * (size_t)i], sc[4 * (size_t)i + 1], sc[4 * (size_t)i + 2], sc[4 * (size_t)i + 3]};
    __shared__ int4 park[2 * 4 * 64];
    const int lane = threadIdx.x;
    valid_park(park, lane, 0, x);
    valid_park(park, lane, 1, y);
    auto ldq = [&](int v) -> Fp28 { return valid_unpark(park, lane, v); };
    JacP p;
    jac_mul(f, p, ldq, k, 4);
    const bool inf = f.is_zero(p.z);
    Fp28 zi = f_inv(p.z);
    Fp28 zi2 = f.sqr(zi);
    Fp28 ax = f.mul(p.x, zi2), ay = f.mul(p.y, f.mul(zi2, zi));
    if (inf) { f_zero(ax); ay = f_const(K28_ONE); }      // identity is (0, 1, infinity), reference src/g1.rs:25-31
    fp28_to_wire(out + 12 * (size_t)i, ax);
    fp28_to_wire(out + 12 * (size_t)i + 6, ay);
    if (out_inf) out_inf[i] = inf ? 1 : 0;
}
__global__ void __launch_bounds__(64, 2) k_g2_mul28(const uint64_t* base, size_t stride, const uint64_t* sc, uint32_t n, uint64_t* out, uint8_t* out_inf) {
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = (int)(tid & 1);
    uint32_t i = tid >> 1;
    const bool live = i < n;
    if (!live) i = n - 1;
    F2 f{c};
    Fp28 x, y;
    fp28_from_wire(x, base + stride * i + 6 * c);
    fp28_from_wire(y, base + stride * i + 12 + 6 * c);
    const uint64_t k[4] = {sc[4 * (size_t)i], sc[4 * (size_t)i + 1], sc[4 * (size_t)i + 2], sc[4 * (size_t)i + 3]};
    __shared__ int4 park[2 * 4 * 64];
    const int lane = threadIdx.x;
    valid_park(park, lane, 0, x);
    valid_park(park, lane, 1, y);
    auto ldq = [&](int v) -> Fp28 { return valid_unpark(park, lane, v); };
    JacP p;
    jac_mul(f, p, ldq, k, 4);
    const bool inf = f.is_zero(p.z);
    // 1 / (z0 + z1 u) = (z0 - z1 u) / (z0^2 + z1^2)   (reference src/fp2.rs:278-296); both lanes invert the norm
    Fp28 o;
    swap_pair(o, p.z);
    Acc acc;
    acc_zero(acc);
    acc_mul(acc, p.z.l, p.z.l);
    acc_mul(acc, o.l, o.l);
    Fp28 nrm;
    acc_reduce(nrm.l, acc);
    Fp28 ninv = f_inv(nrm);
    Fp28 zi = f_mul_v(c ? c_neg(p.z) : p.z, ninv);
    Fp28 zi2 = f.sqr(zi);
    Fp28 ax = f.mul(p.x, zi2), ay = f.mul(p.y, f.mul(zi2, zi));
    if (inf) { f_zero(ax); ay = f.one(); }
    if (live) {
        fp28_to_wire(out + 24 * (size_t)i + 6 * c, ax);
        fp28_to_wire(out + 24 * (size_t)i + 12 + 6 * c, ay);
        if (out_inf && c == 0) out_inf[i] = inf ? 1 : 0;
    }
}

// out = in^-1 for `count` planes of per-check Fp elements: plane j of the input is state element elem_n + j, of the output
// elem_ninv + j (n_checks values each, record stride nc).  The final exponentiation's single inversion is
// (ST_N, ST_NINV, 1), the decompression of the snapshots of an x-power chain (ST_KN, ST_KNINV, 3).  One lane inverts
// B of the count * n_checks values (i, i + L, i + 2L, ...; L lanes) with Montgomery's simultaneous inversion: exclusive
// prefix products parked in the output records, ONE inversion (a^(p-2) in the reference, src/fp.rs:307-319) of the total,
// then two multiplications per value on the way back.
// A zero element (a non-invertible final_exponentiation input, the identity's compressed form) is replaced by one in the
// chain and gets 0, as Fermat gives.
__global__ void __launch_bounds__(64) k_batch_inv(int4* state, uint32_t n_checks_in, uint32_t nc, uint32_t Bf, uint32_t elem_n, uint32_t elem_ninv,
                                                  uint32_t count, NDev nd) {
    const uint32_t n_checks = eff_n(n_checks_in, nd);
    const uint32_t B = Bf & 0x7fffffffu;
    const bool fermat = Bf >> 31;               // cross-check path (ZKP_COOP_INV_FERMAT=1)
    const uint32_t total = n_checks * count;
    const uint32_t L = (total + B - 1) / B;
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= L) return;
    auto recno = [&](uint32_t idx) -> size_t { const uint32_t j = idx / n_checks; return ((size_t)j * nc + (idx - j * n_checks)) * 4; };
    int4* N = state + (size_t)elem_n * nc * 4;
    int4* I = state + (size_t)elem_ninv * nc * 4;
    Fp28 acc = f_const(K28_ONE);
    uint32_t cnt = 0;
    // both loops ask for the next element's records before they work on the current one: a lane's chain is strictly
    // sequential and only a few wavefronts share a SIMD here, so an exposed load latency per step is not covered by anyone
    Fp28 e_next;
    rec_load(e_next, N + recno(i));
#pragma unroll 1
    for (uint32_t idx = i; idx < total && cnt < B; idx += L, cnt++) {
        Fp28 e = e_next;
        if (idx + L < total && cnt + 1 < B) rec_load(e_next, N + recno(idx + L));
        if (B > 1) {
            rec_store(I + recno(idx), acc);
            if (f_is_zero(e)) e = f_const(K28_ONE);
            fp28_mul(acc, acc, e);
        } else {
            acc = e;
        }
    }
    Fp28 inv = fermat ? f_inv_fermat(acc) : f_inv(acc);
    if (B == 1) { rec_store(I + recno(i), inv); return; }
    Fp28 pre_next;
    if (cnt) {
        const size_t at = recno(i + (cnt - 1) * L);
        rec_load(e_next, N + at);
        rec_load(pre_next, I + at);
    }
#pragma unroll 1
    for (uint32_t j = cnt; j-- > 0;) {
        const size_t at = recno(i + j * L);
        Fp28 e = e_next, pre = pre_next, r;
        if (j) {
            const size_t nx = recno(i + (j - 1) * L);
            rec_load(e_next, N + nx);
            rec_load(pre_next, I + nx);
        }
        if (f_is_zero(e)) {
            f_zero(r);
        } else {
            fp28_mul(r, inv, pre);
            fp28_mul(inv, inv, e);
        }
        rec_store(I + at, r);
    }
}

// ---- decompression of snapshots (z2..z5 known, z0 and z1 to recover; Karabina, ePrint 2010/542 Theorem 3.1 in this
// tower's coordinates - tools/coopgen.py checks the identities against the big-integer model):
//     z2 != 0:  z1 = (xi z5^2 + 3 z4^2 - 2 z3) / (4 z2)          z2 == 0:  z1 = 2 z4 z5 / z3   (0 / 0 := 0: the identity)
//     z0 = (2 z1^2 + z2 z5 - 3 z3 z4) xi + 1
// Two lanes per (snapshot, check) - lane parity = Fp2 coefficient, as in k_prep_lines.  k_kdec_a leaves the numerator N in the
// snapshot's z1 records and n = |D|^2 (x 4 where D = z2) in plane elem_n + snapshot; k_batch_inv inverts the planes; k_kdec_b
// finishes: 1 / D = conj(D) / |D|^2.  The denominator D is z2 or z3 itself: since round 5 it is not stored a second time - which of
// the two it is travels in the padding of N's record (third dword of the last quad), and k_kdec_b reads z2 and z3 anyway.
__global__ void __launch_bounds__(64, 2) k_kdec_a(int4* state, uint32_t n_checks_in, uint32_t nc, uint32_t elem_snap, uint32_t count, uint32_t elem_n,
                                                  NDev nd) {
    const uint32_t n_checks = eff_n(n_checks_in, nd);
    if (blockIdx.x * 32u >= n_checks * count) return;
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = (int)(tid & 1);
    uint32_t e = tid >> 1;
    bool live = e < n_checks * count;
    if (!live) e = n_checks * count - 1;
    const uint32_t sn = e / n_checks, check = e - sn * n_checks;
    int4* const st = state + (size_t)check * 4;
    const uint32_t base = elem_snap + 12 * sn;
    auto rec = [&](uint32_t el) -> int4* { return st + (size_t)el * nc * 4; };
    F2 f{c};
    Fp28 z2, z3, z4, z5;
    rec_load(z2, rec(base + 6 + c));
    rec_load(z3, rec(base + 4 + c));
    rec_load(z4, rec(base + 2 + c));
    rec_load(z5, rec(base + 10 + c));
    const bool z2_zero = f.is_zero(z2);
    Fp28 s5 = f.sqr(z5), o;
    swap_pair(o, s5);
    Fp28 na = c ? c_add(o, s5) : c_sub(s5, o);                 // xi z5^2
    Fp28 s4 = f.sqr(z4);
    na = c_sub(c_add(na, c_add(c_dbl(s4), s4)), c_dbl(z3));
    Fp28 nb = na;
    if (__any(z2_zero)) nb = c_dbl(f.mul(z4, z5));             // wave-uniform: almost never taken (z2 = 0: the identity)
    Fp28 N = z2_zero ? nb : na, D = z2_zero ? z3 : z2;
    swap_pair(o, D);
    Acc acc;
    acc_zero(acc);
    acc_mul(acc, D.l, D.l);
    acc_mul(acc, o.l, o.l);
    Fp28 n;
    acc_reduce(n.l, acc);
    if (!z2_zero) n = c_dbl(c_dbl(n));
    if (live) {
        int4* dn = rec(base + 8 + c);
        dn[0] = make_int4(N.l[0], N.l[1], N.l[2], N.l[3]);
        dn[1] = make_int4(N.l[4], N.l[5], N.l[6], N.l[7]);
        dn[2] = make_int4(N.l[8], N.l[9], N.l[10], N.l[11]);
        dn[3] = make_int4(N.l[12], N.l[13], z2_zero ? 1 : 0, 0);       // the tag: D = z3 (1) or z2 (0)
        if (c == 0) rec_store(rec(elem_n + sn), n);
    }
}
__global__ void __launch_bounds__(64, 3) k_kdec_b(int4* state, uint32_t n_checks_in, uint32_t nc, uint32_t elem_snap, uint32_t count, uint32_t elem_ninv,
                                                  NDev nd) {
    const uint32_t n_checks = eff_n(n_checks_in, nd);
    if (blockIdx.x * 32u >= n_checks * count) return;
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = (int)(tid & 1);
    uint32_t e = tid >> 1;
    bool live = e < n_checks * count;
    if (!live) e = n_checks * count - 1;
    const uint32_t sn = e / n_checks, check = e - sn * n_checks;
    int4* const st = state + (size_t)check * 4;
    const uint32_t base = elem_snap + 12 * sn;
    auto rec = [&](uint32_t el) -> int4* { return st + (size_t)el * nc * 4; };
    F2 f{c};
    Fp28 N, D, ninv, z2, z3;
    int d_is_z3;
    {
        const int4* sn_ = rec(base + 8 + c);
        const int4 v0 = sn_[0], v1 = sn_[1], v2 = sn_[2], v3 = sn_[3];
        N.l[0] = v0.x; N.l[1] = v0.y; N.l[2] = v0.z; N.l[3] = v0.w; N.l[4] = v1.x; N.l[5] = v1.y; N.l[6] = v1.z; N.l[7] = v1.w;
        N.l[8] = v2.x; N.l[9] = v2.y; N.l[10] = v2.z; N.l[11] = v2.w; N.l[12] = v3.x; N.l[13] = v3.y;
        d_is_z3 = v3.z;                                                 // k_kdec_a's tag
    }
    rec_load(z2, rec(base + 6 + c));
    rec_load(ninv, rec(elem_ninv + sn));
    D = z2;
    if (__any(d_is_z3 != 0)) {       // wave-uniform and almost never taken (z2 = 0: the identity, pairs with an infinity): D = z3
        Fp28 z3e;
        rec_load(z3e, rec(base + 4 + c));
#pragma unroll
        for (int i = 0; i < NL; i++) D.l[i] = d_is_z3 ? z3e.l[i] : z2.l[i];
    }
    Fp28 dinv = f_mul_v(c ? c_neg(D) : D, ninv);               // conj(D) / |D|^2
    Fp28 z1 = f.mul(N, dinv);
    // t = 2 z1^2 + z2 z5 - 3 z3 z4 under ONE reduction (five products; column budget 2 * 2 * 2 + 2 + 3 * 2 = 16 <= 30; a reduced
    // value, no renormalisation): coefficient c of a b is x1 b + x2 b' with (x1, x2) = (a, -a') or (a', a), ' = the partner's
    Fp28 t;
    {
        Acc acc;
        acc_zero(acc);
        auto mulacc = [&](const Fp28& a, const Fp28& b, int k) {
            Fp28 ao, bo;
            swap_pair(ao, a);
            swap_pair(bo, b);
            int32_t x1[NL], x2[NL];
#pragma unroll
            for (int i = 0; i < NL; i++) {
                x1[i] = k * (c ? ao.l[i] : a.l[i]);
                x2[i] = k * (c ? a.l[i] : -ao.l[i]);
            }
            acc_mul(acc, x1, b.l);
            acc_mul(acc, x2, bo.l);
        };
        {
            Fp28 o1;
            swap_pair(o1, z1);
            int32_t x[NL], y[NL];
#pragma unroll
            for (int i = 0; i < NL; i++) {
                x[i] = 2 * (o1.l[i] + (c ? o1.l[i] : z1.l[i]));
                y[i] = z1.l[i] - (c ? 0 : o1.l[i]);
            }
            acc_mul(acc, x, y);
        }
        {
            Fp28 z5;
            rec_load(z5, rec(base + 10 + c));
            mulacc(z2, z5, 1);
        }
        {
            Fp28 z4;
            rec_load(z3, rec(base + 4 + c));
            rec_load(z4, rec(base + 2 + c));
            mulacc(z3, z4, -3);
        }
        acc_reduce(t.l, acc);
    }
    Fp28 o;
    swap_pair(o, t);
    Fp28 z0 = c ? c_add(o, t) : c_add(c_sub(t, o), f_const(K28_ONE));   // xi t + 1
    z0 = f_vred(z0);
    if (live) {
        rec_store(rec(base + c), z0);
        rec_store(rec(base + 8 + c), z1);
    }
}

// batched field operation on wire operands through the 28-bit core (zkp_fp_op_batch with ZKP_FP_CORE28): 0 mul, 1 add,
// 2 sub, 3 neg, 4 square, 5 invert (0 gives 0).  Reference: Fp::mul / add / sub / neg / square / invert, src/fp.rs:352-455.
__global__ void k_fp28_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp28 x, y, r;
    fp28_from_wire(x, a + 6 * i);
    if (op <= 2) fp28_from_wire(y, b + 6 * i);
    switch (op) {
        case 0: fp28_mul(r, x, y); break;
        case 1: f_add(r, x, y); break;
        case 2: f_sub(r, x, y); break;
        case 3: r = c_neg(x); break;
        case 4: fp28_mul(r, x, x); break;
        default: r = f_inv(x); break;
    }
    fp28_to_wire(out + 6 * i, r);
}

// =============================================================================== group addition and bucket MSM on the 28-bit core
// G1Affine / G2Affine Add (reference src/g1.rs:155-187, src/g2.rs:210-242) in batches, and multi-scalar multiplication by the
// bucket method (zkp_msm.hip drives it; zkp_msm_plan.hpp sizes it).  Same policies as the scalar multiplication: one lane per G1
// value, a lane pair per G2 value (lane c holds coefficient c).  Jacobian values in memory are records of 64 bytes per Fp
// (rec_store), item j of a Jacobian array holds its Fp (coordinate v, coefficient c) at record (3 j + v) NC + c.
namespace msm = zkp::msm;
template <int NC> struct Pol;
template <> struct Pol<1> { using F = F1; };
template <> struct Pol<2> { using F = F2; };

// p += q, both Jacobian (add-2007-bl with Z3 = 2 Z1 Z2 H), with every exceptional case: either input at infinity, P == Q (doubled),
// P == -Q (infinity).  q comes through a loader (0: X, 1: Y, 2: Z) so that it costs no registers across the products; at most six
// values stay live across a by-value call (jac_dbl explains why that matters).
template <class F, class Q>
__device__ __forceinline__ void jac_add(const F& f, JacP& p, Q&& ldq) {
    if (f.is_zero(p.z)) { p.x = ldq(0); p.y = ldq(1); p.z = ldq(2); return; }
    if (f.is_zero(ldq(2))) return;
    Fp28 Z2 = ldq(2);
    Fp28 Z2Z2 = f.sqr(Z2);
    Fp28 U1 = f.mul(p.x, Z2Z2);
    Fp28 S1 = f.mul(p.y, f.mul(Z2, Z2Z2));
    Fp28 ZZ = f.mul(p.z, Z2);
    Fp28 Z1Z1 = f.sqr(p.z);
    Fp28 H = c_sub(f.mul(ldq(0), Z1Z1), U1);
    Fp28 rr = c_sub(f.mul(ldq(1), f.mul(p.z, Z1Z1)), S1);
    if (f.is_zero(H)) {
        if (f.is_zero(rr)) { p.x = ldq(0); p.y = ldq(1); p.z = ldq(2); jac_dbl(f, p); return; }
        f_zero(p.z);   // P + (-P)
        return;
    }
    rr = c_dbl(rr);
    Fp28 I = f.sqr(c_dbl(H));
    Fp28 Z3 = f.mul(c_dbl(ZZ), H);
    Fp28 J = f.mul(H, I);
    Fp28 V = f.mul(U1, I);
    Fp28 X3 = c_sub(c_sub(c_sub(f.sqr(rr), J), V), V);
    Fp28 Y3 = c_sub(f.mul(rr, c_sub(V, X3)), c_dbl(f.mul(S1, J)));
    p.x = f_vred(X3); p.y = f_vred(Y3); p.z = f_vred(Z3);
}

__device__ __forceinline__ void jac_set_inf(const F1& f, JacP& p) { p.x = f.one(); p.y = f.one(); f_zero(p.z); }
__device__ __forceinline__ void jac_set_inf(const F2& f, JacP& p) { p.x = f.one(); p.y = f.one(); f_zero(p.z); }

template <int NC>
__device__ __forceinline__ Fp28 jrec_ld(const int4* j, uint32_t item, int v, int c) {
    Fp28 x;
    rec_load(x, j + ((size_t)item * 3 * NC + (size_t)(v * NC + c)) * 4);
    return x;
}
template <int NC>
__device__ __forceinline__ void jrec_st(int4* j, uint32_t item, int c, const JacP& p) {
    int4* d = j + (size_t)item * 3 * NC * 4;
    rec_store(d + (0 * NC + c) * 4, p.x);
    rec_store(d + (1 * NC + c) * 4, p.y);
    rec_store(d + (2 * NC + c) * 4, p.z);
}
// a Jacobian value parked in LDS, slots v0 .. v0 + 2 (layout of valid_park)
__device__ __forceinline__ void jac_park(int4* park, int lane, int v0, const JacP& p) {
    valid_park(park, lane, v0, p.x);
    valid_park(park, lane, v0 + 1, p.y);
    valid_park(park, lane, v0 + 2, p.z);
}
__device__ __forceinline__ JacP jac_unpark(const int4* park, int lane, int v0) {
    JacP p;
    p.x = valid_unpark(park, lane, v0);
    p.y = valid_unpark(park, lane, v0 + 1);
    p.z = valid_unpark(park, lane, v0 + 2);
    return p;
}

// Jacobian item of an array -> LDS slots 0..2: what jac_add reads through valid_unpark (a loader from global memory lets the compiler
// keep the loaded values in registers across the products, and the addition spills)
template <int NC>
__device__ __forceinline__ void jrec_park(int4* park, int lane, const int4* j, uint32_t item, int c) {
    valid_park(park, lane, 0, jrec_ld<NC>(j, item, 0, c));
    valid_park(park, lane, 1, jrec_ld<NC>(j, item, 1, c));
    valid_park(park, lane, 2, jrec_ld<NC>(j, item, 2, c));
}

// Jacobian -> affine Montgomery (one inversion; the identity becomes (0, 1), reference src/g1.rs:25-31, src/g2.rs:25-31)
__device__ __forceinline__ bool jac_affine(const F1& f, const JacP& p, Fp28& ax, Fp28& ay) {
    const bool inf = f.is_zero(p.z);
    Fp28 zi = f_inv(p.z);
    Fp28 zi2 = f.sqr(zi);
    ax = f.mul(p.x, zi2);
    ay = f.mul(p.y, f.mul(zi2, zi));
    if (inf) { f_zero(ax); ay = f.one(); }
    return inf;
}
__device__ __forceinline__ bool jac_affine(const F2& f, const JacP& p, Fp28& ax, Fp28& ay) {
    const bool inf = f.is_zero(p.z);
    // 1 / (z0 + z1 u) = (z0 - z1 u) / (z0^2 + z1^2)   (reference src/fp2.rs:278-296); both lanes invert the norm
    Fp28 o;
    swap_pair(o, p.z);
    Acc acc;
    acc_zero(acc);
    acc_mul(acc, p.z.l, p.z.l);
    acc_mul(acc, o.l, o.l);
    Fp28 nrm;
    acc_reduce(nrm.l, acc);
    Fp28 ninv = f_inv(nrm);
    Fp28 zi = f_mul_v(f.c ? c_neg(p.z) : p.z, ninv);
    Fp28 zi2 = f.sqr(zi);
    ax = f.mul(p.x, zi2);
    ay = f.mul(p.y, f.mul(zi2, zi));
    if (inf) { f_zero(ax); ay = f.one(); }
    return inf;
}

// out[i] = a[i] + b[i], affine in / affine out.  inf_a / inf_b / out_inf may be null.
template <int NC>
__global__ void __launch_bounds__(64, 2) k_add28(const uint64_t* a, const uint8_t* ia, const uint64_t* b, const uint8_t* ib, uint32_t n,
                                                 uint64_t* out, uint8_t* out_inf) {
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = NC == 2 ? (int)(tid & 1) : 0;
    uint32_t i = tid / NC;
    const bool live = i < n;
    if (!live) i = n - 1;
    typename Pol<NC>::F f{c};
    constexpr int PW = 12 * NC;
    const int lane = threadIdx.x;
    __shared__ int4 park[2 * 4 * 64];
    JacP p;
    fp28_from_wire(p.x, a + PW * (size_t)i + 6 * c);
    fp28_from_wire(p.y, a + PW * (size_t)i + 6 * NC + 6 * c);
    p.z = f.one();
    if (ia && ia[i]) f_zero(p.z);
    if (!(ib && ib[i])) {
        Fp28 qx, qy;
        fp28_from_wire(qx, b + PW * (size_t)i + 6 * c);
        fp28_from_wire(qy, b + PW * (size_t)i + 6 * NC + 6 * c);
        valid_park(park, lane, 0, qx);
        valid_park(park, lane, 1, qy);
        jac_madd(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, v); });
    }
    Fp28 ax, ay;
    const bool inf = jac_affine(f, p, ax, ay);
    if (live) {
        fp28_to_wire(out + PW * (size_t)i + 6 * c, ax);
        fp28_to_wire(out + PW * (size_t)i + 6 * NC + 6 * c, ay);
        if (out_inf && c == 0) out_inf[i] = inf ? 1 : 0;
    }
}

// out[i] = [a] P + [b] phi'(P), phi'(P) = (beta x, -y), a and b 64-bit: for P in G1, phi'(P) = [z^2] P (the relation k_g1_valid28
// tests), so out[i] = [a + b z^2] P - a 128-bit scalar multiplication in 64 doublings (zkp_g1_mul_endo_batch, the batch check's scaling).
// One lane per point; points i share the (a, b) of ab[2 (i / per)].  Joint double-and-add over the 64 bit pairs with the table P, phi'(P),
// T = P + phi'(P) in LDS: every lane adds ITS entry through one full addition (jac_add, every exceptional case; T is Jacobian, and infinite
// when phi'(P) = -P), so a wavefront runs one addition per bit pair whatever its lanes' bits.  phi'(P) is not stored: its x costs one
// product at the load (five LDS slots, 20 KB: two workgroups per SIMD as the launch bounds ask).
__global__ void __launch_bounds__(64, 2) k_g1_mul_endo28(const uint64_t* base, const uint8_t* inf, const uint64_t* ab, uint32_t n, uint32_t per,
                                                         uint64_t* out, uint8_t* out_inf) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    F1 f{0};
    const int lane = threadIdx.x;
    __shared__ int4 park[5 * 4 * 64];   // 0 x, 1 y of P; 2..4 T (Jacobian)
    const uint32_t g = i / per;
    const uint64_t a = ab[2 * (size_t)g], b = ab[2 * (size_t)g + 1];
    JacP p;
    fp28_from_wire(p.x, base + 12 * (size_t)i);
    fp28_from_wire(p.y, base + 12 * (size_t)i + 6);
    valid_park(park, lane, 0, p.x);
    valid_park(park, lane, 1, p.y);
    p.z = f.one();
    jac_madd(f, p, [&](int v) -> Fp28 { return v == 0 ? f.mul(valid_unpark(park, lane, 0), f_const(K28_BETA)) : c_neg(valid_unpark(park, lane, 1)); });
    jac_park(park, lane, 2, p);
    jac_set_inf(f, p);
    if (!(inf && inf[i])) {
#pragma unroll 1
        for (int bit = 63; bit >= 0; bit--) {
            jac_dbl(f, p);
            const int sel = (int)((a >> bit) & 1) | (int)((b >> bit) & 1) << 1;   // 1: P, 2: phi'(P), 3: T
            if (sel)
                jac_add(f, p, [&](int v) -> Fp28 {
                    if (sel == 3) return valid_unpark(park, lane, 2 + v);
                    if (v == 2) return f.one();
                    const Fp28 q = valid_unpark(park, lane, v);
                    if (sel == 1) return q;
                    return v == 0 ? f.mul(q, f_const(K28_BETA)) : c_neg(q);
                });
        }
    }
    Fp28 ax, ay;
    const bool pinf = jac_affine(f, p, ax, ay);
    fp28_to_wire(out + 12 * (size_t)i, ax);
    fp28_to_wire(out + 12 * (size_t)i + 6, ay);
    if (out_inf) out_inf[i] = pinf ? 1 : 0;
}

// rec[i] = [a_i + b_i z^2] P_i as a JACOBIAN record (zkp_bls_grouped.hip: the scaled keys go straight into the accumulation levels of
// the bucket MSM, msm_accum(1, false, ...), so they never need to be affine).  k_g1_mul_endo28's joint double-and-add with its table in
// LDS and the full jac_add, one (a, b) per point; no jac_affine and no wire conversion at the end: about 461 of the 1,500 products of
// that kernel go.  A point at infinity and a zero (a, b) store the identity (1, 1, 0).
__global__ void __launch_bounds__(64, 2) k_grp_scale(const uint64_t* base, const uint8_t* inf, const uint64_t* ab, uint32_t n, int4* rec) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    F1 f{0};
    const int lane = threadIdx.x;
    __shared__ int4 park[5 * 4 * 64];   // 0 x, 1 y of P; 2..4 T (Jacobian)
    const uint64_t a = ab[2 * (size_t)i], b = ab[2 * (size_t)i + 1];
    JacP p;
    fp28_from_wire(p.x, base + 12 * (size_t)i);
    fp28_from_wire(p.y, base + 12 * (size_t)i + 6);
    valid_park(park, lane, 0, p.x);
    valid_park(park, lane, 1, p.y);
    p.z = f.one();
    jac_madd(f, p, [&](int v) -> Fp28 { return v == 0 ? f.mul(valid_unpark(park, lane, 0), f_const(K28_BETA)) : c_neg(valid_unpark(park, lane, 1)); });
    jac_park(park, lane, 2, p);
    jac_set_inf(f, p);
    if (!(inf && inf[i])) {
#pragma unroll 1
        for (int bit = 63; bit >= 0; bit--) {
            jac_dbl(f, p);
            const int sel = (int)((a >> bit) & 1) | (int)((b >> bit) & 1) << 1;   // 1: P, 2: phi'(P), 3: T
            if (sel)
                jac_add(f, p, [&](int v) -> Fp28 {
                    if (sel == 3) return valid_unpark(park, lane, 2 + v);
                    if (v == 2) return f.one();
                    const Fp28 q = valid_unpark(park, lane, v);
                    if (sel == 1) return q;
                    return v == 0 ? f.mul(q, f_const(K28_BETA)) : c_neg(q);
                });
        }
    }
    jrec_st<1>(rec, i, 0, p);
}

// =============================================================================== the G1 NTT and the FK20 scalar products (zkp_fk20.hip drives
// them; zkp_fk20_plan.hpp holds every index).  One lane per butterfly, Jacobian records (jrec_*) in a workspace between the stages, every
// stage in place: a lane reads and writes the same two records.
namespace fk = zkp::fk20;

// p <- [a + b z^2] p for a JACOBIAN p in G1 and a, b of 128 bits: k_g1_mul_endo28's joint double-and-add, 128 doublings, with the table
// Q = p (LDS slots 0..2), phi'(Q) = (beta X, -Y, Z) (not stored: one product at the load) and T = Q + phi'(Q) (slots 3..5).  Every addition
// is the full jac_add: Q may be infinite, T is infinite when phi'(Q) = -Q, and the accumulator meets +-Q on ordinary inputs.
__device__ __forceinline__ void jac_mul_split(const F1& f, JacP& p, int4* park, int lane, uint64_t a_lo, uint64_t a_hi, uint64_t b_lo, uint64_t b_hi) {
    jac_park(park, lane, 0, p);
    jac_add(f, p, [&](int v) -> Fp28 {
        const Fp28 q = valid_unpark(park, lane, v);
        return v == 0 ? f.mul(q, f_const(K28_BETA)) : v == 1 ? c_neg(q) : q;
    });
    jac_park(park, lane, 3, p);
    jac_set_inf(f, p);
#pragma unroll 1
    for (int h = 1; h >= 0; h--) {
        const uint64_t a = h ? a_hi : a_lo, b = h ? b_hi : b_lo;
#pragma unroll 1
        for (int bit = 63; bit >= 0; bit--) {
            jac_dbl(f, p);
            const int sel = (int)((a >> bit) & 1) | (int)((b >> bit) & 1) << 1;   // 1: Q, 2: phi'(Q), 3: T
            if (sel)
                jac_add(f, p, [&](int v) -> Fp28 {
                    if (sel == 3) return valid_unpark(park, lane, 3 + v);
                    const Fp28 q = valid_unpark(park, lane, v);
                    if (sel == 1 || v == 2) return q;
                    return v == 0 ? f.mul(q, f_const(K28_BETA)) : c_neg(q);
                });
        }
    }
}

__device__ __forceinline__ JacP jrec_get(const int4* rec, uint32_t item) {
    JacP p;
    p.x = jrec_ld<1>(rec, item, 0, 0);
    p.y = jrec_ld<1>(rec, item, 1, 0);
    p.z = jrec_ld<1>(rec, item, 2, 0);
    return p;
}

// The stage on bit 0 (twiddle one, no product): A + B and A - B of the two inputs of a lane, read where fk::first_source says - the
// caller's wire points and flags in its order, the FK20 setup vector, or records of the workspace - and stored as records.  k = 0: a copy.
template <int MODE>
__global__ void __launch_bounds__(64, 2) k_g1ntt_first(const uint64_t* in, const uint8_t* inf, int4* rec, fk::First a) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n_lane) return;
    F1 f{0};
    const int lane = threadIdx.x;
    __shared__ int4 park[3 * 4 * 64];   // B: affine (slots 0, 1) from the wire, Jacobian from records
    const uint32_t k = a.at.k, j = k ? t >> (k - 1) : t, e0 = k ? (t & fk::low_mask(k - 1)) << 1 : 0;
    const int64_t sa = fk::first_source(a, j, e0), sb = k ? fk::first_source(a, j, e0 + 1) : fk::SRC_INFINITY;
    const uint32_t r0 = fk::span_record(a.at, j, e0);
    JacP p;
    bool b_inf;
    if (MODE == fk::SRC_REC) {
        p = jrec_get(rec, (uint32_t)sa);
        b_inf = sb == fk::SRC_INFINITY;
        if (!b_inf) jrec_park<1>(park, lane, rec, (uint32_t)sb, 0);
    } else {
        jac_set_inf(f, p);
        if (sa != fk::SRC_INFINITY && !(inf && inf[sa])) {
            fp28_from_wire(p.x, in + 12 * (size_t)sa);
            fp28_from_wire(p.y, in + 12 * (size_t)sa + 6);
            p.z = f.one();
        }
        b_inf = sb == fk::SRC_INFINITY || (inf && inf[sb]);
        if (!b_inf) {
            Fp28 qx, qy;
            fp28_from_wire(qx, in + 12 * (size_t)sb);
            fp28_from_wire(qy, in + 12 * (size_t)sb + 6);
            valid_park(park, lane, 0, qx);
            valid_park(park, lane, 1, qy);
        }
    }
    if (!k) { jrec_st<1>(rec, r0, 0, p); return; }
    if (b_inf) {           // A + inf = A - inf = A
        jrec_st<1>(rec, r0, 0, p);
        jrec_st<1>(rec, r0 + 1, 0, p);
        return;
    }
    JacP d = p;
    if (MODE == fk::SRC_REC) {
        jac_add(f, d, [&](int v) -> Fp28 { const Fp28 q = valid_unpark(park, lane, v); return v == 1 ? c_neg(q) : q; });
        jrec_st<1>(rec, r0 + 1, 0, d);
        p = jrec_get(rec, (uint32_t)sa);
        jac_add(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, v); });
    } else {
        jac_madd(f, d, [&](int v) -> Fp28 { const Fp28 q = valid_unpark(park, lane, v); return v == 1 ? c_neg(q) : q; });
        jrec_st<1>(rec, r0 + 1, 0, d);
        jac_set_inf(f, p);
        if (sa != fk::SRC_INFINITY && !(inf && inf[sa])) {
            fp28_from_wire(p.x, in + 12 * (size_t)sa);
            fp28_from_wire(p.y, in + 12 * (size_t)sa + 6);
            p.z = f.one();
        }
        jac_madd(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, v); });
    }
    jrec_st<1>(rec, r0, 0, p);
}

// A twiddled stage: T = [w^t] B through the split twiddle of the context's table, then A - T and A + T, both by the full addition with T
// in LDS.  B's record takes A - T before A's takes A + T: A is read twice, never kept across the products.
__global__ void __launch_bounds__(64, 2) k_g1ntt_stage(int4* rec, const uint64_t* __restrict__ split, fk::Stage a) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n_bfly) return;
    F1 f{0};
    const int lane = threadIdx.x;
    __shared__ int4 park[6 * 4 * 64];
    uint32_t r0, r1, tw;
    fk::stage_lane(a, t, &r0, &r1, &tw);
    const uint64_t a_lo = split[4 * (size_t)tw], a_hi = split[4 * (size_t)tw + 1], b_lo = split[4 * (size_t)tw + 2], b_hi = split[4 * (size_t)tw + 3];
    JacP p = jrec_get(rec, r1);
    jac_mul_split(f, p, park, lane, a_lo, a_hi, b_lo, b_hi);
    jac_park(park, lane, 0, p);
    p = jrec_get(rec, r0);
    jac_add(f, p, [&](int v) -> Fp28 { const Fp28 q = valid_unpark(park, lane, v); return v == 1 ? c_neg(q) : q; });
    jrec_st<1>(rec, r1, 0, p);
    p = jrec_get(rec, r0);
    jac_add(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, v); });
    jrec_st<1>(rec, r0, 0, p);
}

// the inverse transform's [N^-1]: one more split multiplication of every record, in place
__global__ void __launch_bounds__(64, 2) k_g1ntt_scale(int4* rec, fk::Out a, uint64_t a_lo, uint64_t a_hi, uint64_t b_lo, uint64_t b_hi) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n_pt) return;
    F1 f{0};
    const int lane = threadIdx.x;
    __shared__ int4 park[6 * 4 * 64];
    uint32_t r;
    uint64_t slot;
    fk::out_lane(a, t, &r, &slot);
    JacP p = jrec_get(rec, r);
    jac_mul_split(f, p, park, lane, a_lo, a_hi, b_lo, b_hi);
    jrec_st<1>(rec, r, 0, p);
}
// record -> wire point and flag, in the order the caller asked for: one inversion per output
__global__ void __launch_bounds__(64, 2) k_g1ntt_out(const int4* rec, uint64_t* out, uint8_t* out_inf, fk::Out a) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n_pt) return;
    F1 f{0};
    uint32_t r;
    uint64_t slot;
    fk::out_lane(a, t, &r, &slot);
    const JacP p = jrec_get(rec, r);
    Fp28 ax, ay;
    const bool pinf = jac_affine(f, p, ax, ay);
    fp28_to_wire(out + 12 * slot, ax);
    fp28_to_wire(out + 12 * slot + 6, ay);
    out_inf[slot] = pinf ? 1 : 0;
}

// FK20's 2 N products per polynomial: record t <- [fr[t]] setup[bitrev(t mod 2 N)].  The scalars are the size-2N Fr transform in
// bit-reversed order, so record t holds what the decimation in time wants at position t.  k_g1_mul28's chain on an affine base; no
// conversion back: the result stays Jacobian.  An infinite setup point gives the identity.
__global__ void __launch_bounds__(64, 2) k_fk20_mul(const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* sc, uint32_t n_pt, uint32_t k1,
                                                    int4* rec) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_pt) return;
    F1 f{0};
    const int lane = threadIdx.x;
    __shared__ int4 park[2 * 4 * 64];
    const uint32_t src = fk::bitrev(t & fk::low_mask(k1), k1);
    JacP p;
    jac_set_inf(f, p);
    if (!(setup_inf && setup_inf[src])) {
        Fp28 x, y;
        fp28_from_wire(x, setup + 12 * (size_t)src);
        fp28_from_wire(y, setup + 12 * (size_t)src + 6);
        valid_park(park, lane, 0, x);
        valid_park(park, lane, 1, y);
        const uint64_t sk[4] = {sc[4 * (size_t)t], sc[4 * (size_t)t + 1], sc[4 * (size_t)t + 2], sc[4 * (size_t)t + 3]};
        jac_mul(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, v); }, sk, 4);
    }
    jrec_st<1>(rec, t, 0, p);
}

// =============================================================================== the KZG cell proofs' multiply-accumulate (zkp_cells.hip drives it;
// zkp_cells_plan.hpp holds every index).  Slot t of a polynomial is H[t] = sum_{i < l} [c^_i[t]] X_i[t]: the l bases of a slot are summed
// anyway, so the g = 2^s bases of a lane share ONE chain of 255 doublings.  The bases are affine setup points, converted once and parked in
// LDS (slots 2 q, 2 q + 1 of base q: 8 KiB per base and workgroup, dynamic, so a launch reserves g x 8 KiB and g = 1 keeps eight
// workgroups per CU); the scalars are read a byte of each at a time into one register, so a bit test is a shift.  At every bit the lane
// adds each base whose scalar has the bit by the mixed addition with every exceptional case (jac_madd): zero coefficients leave the
// accumulator infinite for many bits; two bases of a lane that are equal or opposite (a setup with tau = 1 or tau = -1) under equal scalars
// make it meet +X (the doubling) and -X (infinity) at the first bit they share; a base flagged infinite (k = 1: all of them) has its
// bits masked away.  The result stays Jacobian: a partial, or the record when g = l.
namespace cl = zkp::cells;
__global__ void __launch_bounds__(64, 2) k_cell_mac(const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* sc, int4* part, int4* rec, cl::Mac a) {
    const uint32_t id = blockIdx.x * 64 + threadIdx.x;
    if (id >= a.n_lane) return;
    F1 f{0};
    const int lane = threadIdx.x;
    extern __shared__ int4 park[];           // cl::mac_lds_bytes(a.s)
    uint32_t j, t, i0;
    cl::mac_lane(a, id, &j, &t, &i0);
    const uint32_t g = 1u << a.s;
    uint32_t live = 0;
#pragma unroll 1
    for (uint32_t q = 0; q < g; q++) {
        const uint32_t src = cl::mac_base(a, t, i0 + q);
        if (setup_inf && setup_inf[src]) continue;
        Fp28 x, y;
        fp28_from_wire(x, setup + 12 * (size_t)src);
        fp28_from_wire(y, setup + 12 * (size_t)src + 6);
        valid_park(park, lane, 2 * q, x);
        valid_park(park, lane, 2 * q + 1, y);
        live |= 0xffu << (8 * q);
    }
    const uint8_t* scb = (const uint8_t*)sc;
    JacP p;
    jac_set_inf(f, p);
    if (live) {
#pragma unroll 1
        for (int by = 31; by >= 0; by--) {
            uint32_t pk = 0;
#pragma unroll 1
            for (uint32_t q = 0; q < g; q++) pk |= (uint32_t)scb[32 * cl::mac_scalar(a, j, t, i0 + q) + by] << (8 * q);
            pk &= live;
#pragma unroll 1
            for (int b = 7; b >= 0; b--) {
                jac_dbl(f, p);
                if (!((pk >> b) & 0x01010101u)) continue;
#pragma unroll 1
                for (uint32_t q = 0; q < g; q++)
                    if ((pk >> (8 * q + b)) & 1) jac_madd(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, 2 * q + v); });
            }
        }
    }
    if (a.s == a.log2_l) jrec_st<1>(rec, cl::mac_record(a, j, t), 0, p);
    else jrec_st<1>(part, id, 0, p);
}
// record (j, t) <- the sum of the slot's l / g partials, by the full addition.  Infinite partials occur on ordinary inputs (zero
// coefficients); equal and opposite ones need strides whose bases AND scalars agree up to sign - equal coefficients under a setup with
// tau = 1 (every X_i the same) or tau = -1 (X_i alternating in sign) - which tests/test_gpu_cells.py runs.  Equal coefficients alone do not
// give them: X_i[t] = tau^-i X_0[t]
__global__ void __launch_bounds__(64, 2) k_cell_sum(const int4* part, int4* rec, cl::Sum a) {
    const uint32_t id = blockIdx.x * 64 + threadIdx.x;
    if (id >= a.n_lane) return;
    F1 f{0};
    const int lane = threadIdx.x;
    __shared__ int4 park[3 * 4 * 64];
    const uint32_t gl = a.log2_l - a.s, first = id << gl;
    JacP p = jrec_get(part, first);
#pragma unroll 1
    for (uint32_t q = 1; q < (1u << gl); q++) {
        jrec_park<1>(park, lane, part, first + q, 0);
        jac_add(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, v); });
    }
    jrec_st<1>(rec, ((id >> a.k1) << a.blk) + (id & fk::low_mask(a.k1)), 0, p);
}

// ---- MSM 1: n wire Fp elements -> Montgomery records (the points' coordinates, converted once per pass)
__global__ void __launch_bounds__(256) k_msm_points(const uint64_t* w, uint32_t n_fp, int4* rec) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_fp) return;
    Fp28 x;
    fp28_from_wire(x, w + 6 * (size_t)i);
    rec_store(rec + 4 * (size_t)i, x);
}

// ---- MSM 2: signed c-bit digits of every term's scalar, one sort key and one value per (term, window).  Digit d of window w is
// bits [w c, w c + c) plus the carry of window w - 1, moved to d - 2^c (carry 1) when above 2^(c-1): k = sum_w d_w 2^(c w) exactly,
// |d| <= 2^(c-1), and the top window (fewer than c bits of the scalar) never carries out.  key: bucket (s W + w) 2^(c-1) + |d| - 1, or
// KEY_NONE for d = 0 and for points at infinity; value: the point's index in the pass's records, bit 31 the digit's sign.
__global__ void __launch_bounds__(256) k_msm_digits(const uint64_t* sc, const uint8_t* inf, uint32_t terms, uint32_t m, int shared, uint32_t c,
                                                    uint32_t windows, uint32_t* keys, uint32_t* vals) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= terms) return;
    const uint32_t seg = t / m, pt = shared ? t - seg * m : t;
    const bool dead = inf && inf[pt];
    const uint64_t k[4] = {sc[4 * (size_t)t], sc[4 * (size_t)t + 1], sc[4 * (size_t)t + 2], sc[4 * (size_t)t + 3]};
    const int32_t half = 1 << (c - 1);
    int32_t carry = 0;
#pragma unroll 1
    for (uint32_t w = 0; w < windows; w++) {
        const uint32_t pos = w * c, wd = pos >> 6, sh = pos & 63;
        uint64_t v = wd < 4 ? k[wd] >> sh : 0;
        if (sh + c > 64 && wd + 1 < 4) v |= k[wd + 1] << (64 - sh);
        int32_t d = (int32_t)(v & ((1u << c) - 1)) + carry;
        carry = d > half ? 1 : 0;
        if (carry) d -= 2 * half;
        const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
        const size_t o = (size_t)w * terms + t;
        keys[o] = (d == 0 || dead) ? msm::KEY_NONE : ((seg * windows + w) << (c - 1)) + mag - 1;
        vals[o] = pt | (d < 0 ? 0x80000000u : 0u);
    }
}

// ---- MSM 3: segmented sum of sorted entries, RUN entries per lane (G1) / lane pair (G2) whatever the bucket sizes.  A key group that
// starts and ends inside the run is complete: its sum goes to sums[key] (at level 0 always; later only when the group holds a real
// partial, KEY_FLAG).  The run's first group when it began in an earlier run, and its last when it goes on in a later one, leave
// partial sums in the run's two output slots instead (an unused slot: infinity under a neighbouring key, no flag, so the output stays
// sorted).  The next level sums those; the last level has one run.  L0: the entries are (key, signed point index) and the sum is of
// mixed additions; otherwise Jacobian partial sums (jac_add).
template <int NC, bool L0>
__global__ void __launch_bounds__(64, 2) k_msm_accum(const uint32_t* keys, const uint32_t* vals, const int4* src, uint32_t n, uint32_t n_sums,
                                                     int4* sums, uint32_t* okeys, int4* oj) {
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = NC == 2 ? (int)(tid & 1) : 0;
    const uint32_t runs = (n + msm::RUN - 1) / msm::RUN;
    uint32_t t = tid / NC;
    const bool live = t < runs;
    if (!live) t = runs - 1;
    const uint32_t lo = t * msm::RUN, hi = n - lo < msm::RUN ? n : lo + msm::RUN;
    constexpr uint32_t KM = ~msm::KEY_FLAG;
    const uint32_t prev = lo ? keys[lo - 1] & KM : 0xffffffffu, next = hi < n ? keys[hi] & KM : 0xffffffffu;
    typename Pol<NC>::F f{c};
    const int lane = threadIdx.x;
    __shared__ int4 park[3 * 4 * 64];
    JacP acc;
    jac_set_inf(f, acc);
    uint32_t cur = keys[lo] & KM, s0k = 0, s1k = 0;
    bool any = L0, first = true, s0 = false, s1 = false;
    auto emit = [&](bool ends) {
        if (cur >= n_sums) return;
        const bool starts = !(first && prev == cur);
        const uint32_t kw = cur | (any ? msm::KEY_FLAG : 0u);
        if (starts && ends) {
            if (any && live) jrec_st<NC>(sums, cur, c, acc);
        } else if (!starts) {
            s0 = true; s0k = kw;
            if (live) jrec_st<NC>(oj, 2 * t, c, acc);
        } else {
            s1 = true; s1k = kw;
            if (live) jrec_st<NC>(oj, 2 * t + 1, c, acc);
        }
    };
#pragma unroll 1
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t kw = keys[i], k = kw & KM;
        if (k != cur) {
            emit(true);
            first = false;
            cur = k;
            jac_set_inf(f, acc);
            any = L0;
        }
        if (k >= n_sums) break;   // dropped digits sort last: nothing behind them
        if (L0) {
            const uint32_t v = vals[i], idx = v & 0x7fffffffu;
            Fp28 qx, qy;
            rec_load(qx, src + ((size_t)idx * 2 * NC + c) * 4);
            rec_load(qy, src + ((size_t)idx * 2 * NC + NC + c) * 4);
            if (v >> 31) qy = c_neg(qy);
            valid_park(park, lane, 0, qx);
            valid_park(park, lane, 1, qy);
            jac_madd(f, acc, [&](int w) -> Fp28 { return valid_unpark(park, lane, w); });
        } else {
            any = any || (kw & msm::KEY_FLAG);
            jrec_park<NC>(park, lane, src, i, c);
            jac_add(f, acc, [&](int w) -> Fp28 { return valid_unpark(park, lane, w); });
        }
    }
    emit(next != cur);
    if (!live) return;
    JacP z;
    jac_set_inf(f, z);
    if (!s0) jrec_st<NC>(oj, 2 * t, c, z);
    if (!s1) jrec_st<NC>(oj, 2 * t + 1, c, z);
    if (c == 0) {
        okeys[2 * t] = s0 ? s0k : (s1 ? s1k & KM : cur);
        okeys[2 * t + 1] = s1 ? s1k : (s0 ? s0k & KM : cur);
    }
}

// ---- MSM 4: bucket reduction, sum_j (j + 1) B_j of one window split over `split` lanes (pairs): lane s takes buckets [s L, s L + L),
// L = chunk, with two running sums (run = sum_{j' >= j} B_j', acc = sum of the runs = sum (j - s L + 1) B_j) and adds (s L) run.  Both
// sums are parked in LDS between the additions.  Output: one flagged partial per lane under key window, for the fix-up levels.
template <int NC>
__global__ void __launch_bounds__(64, 2) k_msm_reduce(const int4* buckets, uint32_t n_sums, uint32_t split, uint32_t chunk, uint32_t* okeys,
                                                      int4* oj) {
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = NC == 2 ? (int)(tid & 1) : 0;
    uint32_t u = tid / NC;
    const bool live = u < n_sums * split;
    if (!live) u = n_sums * split - 1;
    const uint32_t win = u / split, s = u - win * split, base = win * split * chunk + s * chunk;
    typename Pol<NC>::F f{c};
    const int lane = threadIdx.x;
    __shared__ int4 park[6 * 4 * 64];
    JacP p;
    jac_set_inf(f, p);
    jac_park(park, lane, 0, p);   // run
    jac_park(park, lane, 3, p);   // acc
#pragma unroll 1
    for (uint32_t j = chunk; j-- > 0;) {
        p = jac_unpark(park, lane, 0);
        jac_add(f, p, [&](int v) -> Fp28 { return jrec_ld<NC>(buckets, base + j, v, c); });
        jac_park(park, lane, 0, p);
        p = jac_unpark(park, lane, 3);
        jac_add(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, v); });
        jac_park(park, lane, 3, p);
    }
    const uint32_t e = s * chunk;
    if (e) {
        p = jac_unpark(park, lane, 0);
        const int top = 31 - __builtin_clz(e);
#pragma unroll 1
        for (int b = top - 1; b >= 0; b--) {
            jac_dbl(f, p);
            if ((e >> b) & 1) jac_add(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, v); });
        }
        jac_add(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, 3 + v); });
    } else {
        p = jac_unpark(park, lane, 3);
    }
    if (!live) return;
    jrec_st<NC>(oj, u, c, p);
    if (c == 0) okeys[u] = win | msm::KEY_FLAG;
}

// ---- MSM 5: per segment, sum_w 2^(c w) S_w by Horner (c doublings per window), then one inversion to affine wire output
template <int NC>
__global__ void __launch_bounds__(64, 2) k_msm_final(const int4* wsums, uint32_t segs, uint32_t windows, uint32_t c_bits, uint64_t* out,
                                                     uint8_t* out_inf) {
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = NC == 2 ? (int)(tid & 1) : 0;
    uint32_t sg = tid / NC;
    const bool live = sg < segs;
    if (!live) sg = segs - 1;
    typename Pol<NC>::F f{c};
    const int lane = threadIdx.x;
    __shared__ int4 park[3 * 4 * 64];
    JacP p;
    jac_set_inf(f, p);
#pragma unroll 1
    for (uint32_t w = windows; w-- > 0;) {
        if (w + 1 < windows)
#pragma unroll 1
            for (uint32_t b = 0; b < c_bits; b++) jac_dbl(f, p);
        jrec_park<NC>(park, lane, wsums, sg * windows + w, c);
        jac_add(f, p, [&](int v) -> Fp28 { return valid_unpark(park, lane, v); });
    }
    Fp28 ax, ay;
    const bool inf = jac_affine(f, p, ax, ay);
    constexpr int PW = 12 * NC;
    if (live) {
        fp28_to_wire(out + PW * (size_t)sg + 6 * c, ax);
        fp28_to_wire(out + PW * (size_t)sg + 6 * NC + 6 * c, ay);
        if (out_inf && c == 0) out_inf[sg] = inf ? 1 : 0;
    }
}

// the primer of prime(): a grid of one-wavefront workgroups that leave at once
__global__ void __launch_bounds__(64) k_primer() {}

}  // namespace

// =============================================================================== host side
namespace zkp {

struct CoopProgDev { uint32_t* hdr; uint32_t* tbl; uint4* rtbl; uint32_t nslot; uint32_t nconst; uint32_t wide; };
constexpr int MAX_PIPES = plan::MAX_PIPES;
struct CoopDev;
struct CoopPipe {            // one in-flight chunk: its own workspace and (for pipes > 0) its own stream
    int4* lines;  size_t lines_bytes;
    int4* state;  size_t state_bytes;
    hipStream_t stream;
    hipEvent_t done;
    CoopDev* owner;
    // transient, set on the copy a chunk's launches are given: the check count in device memory and this chunk's offset into the list
    // it counts (coop_pairing's n_dev argument); {nullptr, 0} otherwise
    NDev nd;
};
struct CoopDev {
    CoopProgDev progs[ZKP_PROG_COUNT];
    int4* consts;
    CoopPipe pipe[MAX_PIPES];
    plan::Knobs kn;          // chunking / splitting knobs, clamped (zkp_plan.hpp: the arithmetic the CPU test walks under sanitizers)
    bool inv_fermat;         // a^(p-2) instead of the division-step inversion (cross-check)
    int cus;                 // compute units of the device
    bool prime_now;          // set per super-chunk by two_phase: batches of at most one chunk only (a larger one keeps the GPU full: nothing to place)
    int prime;               // ZKP_COOP_PRIME: small grids in the dispatcher's bad bands are preceded by an empty grid of the same size (prime())
    int4* big_state;         // per-check state of a whole super-chunk (7.9 KB per check)
    size_t big_state_bytes;
    int4* vscratch;          // k_g2_valid_fast3: Montgomery limbs of the affine points (2 values x 4 quads per lane)
    size_t vscratch_bytes;
    hipEvent_t ready;
    // coop_profile_pairing: every launch of one pass bracketed by events on its stream (ONE pipeline, so that no two kernels overlap)
    struct ProfEv { int cls; hipEvent_t a, b; };
    std::vector<ProfEv>* prof;     // null: not profiling
    bool prof_phase_c;
    bool miller1;                  // ZKP_COOP_MILLER1 (default 1): one-pair Miller loops that end in the state record run on k_miller1
    const uint32_t* n_dev;         // for the duration of one coop_pairing call: the device-resident check count (or null)
};

enum { PRIME_PREP, PRIME_KSQ, PRIME_INV };      // kernel classes of prime()
// kernel classes of coop_profile_pairing (include/zkp_pairings.h ZKP_PROFILE_*)
enum { PROF_PREP = 0, PROF_MILLER, PROF_FEXP_A, PROF_INV, PROF_KSQ, PROF_KDEC_A, PROF_KDEC_B, PROF_C_DEEP, PROF_C_PLAIN, PROF_CLASSES };
struct ProfScope {
    CoopDev* d; hipStream_t s; hipEvent_t b = nullptr;
    ProfScope(CoopDev* d_, hipStream_t s_, int cls) : d(d_), s(s_) {      // d may be null: a launch outside any context's profile
        if (!d || !d->prof) return;
        hipEvent_t a = nullptr;
        if (hipEventCreate(&a) != hipSuccess) return;
        if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); b = nullptr; return; }
        (void)hipEventRecord(a, s);
        d->prof->push_back({cls, a, b});
    }
    ~ProfScope() { if (b) (void)hipEventRecord(b, s); }
};

// The MULACC table of a program with every LDS address resolved per LANE (the asm block of k_coop reads it: no address
// arithmetic in the term loop).  Row r = table offset / 12 + term, 64 lanes per row, one uint4 per lane:
//   x = byte address of the A1 record (plane 0), y = B1, z = A2 | B2 << 16, w = 0;
// the row behind a step's last term carries the step's per-lane flag words: x = negate bits (bit t = term t) | doubled-A
// bits << 12, y = subtract-A2 bits | subtract-B2 bits << 12.  Lane -> (group, lane in group) and the slot -> address map are
// k_coop's (gbase, slot_off); lanes 60..63 compute on group 4's addresses and never store.
static void coop_resolve_table(const ZkpProgDesc& p, std::vector<uint4>& rt) {
    const int S = coop_cfg_slots(p.wide), SC = coop_cfg_consts(p.wide);
    const int SG = coop_group_stride(S);
    const size_t rows = p.n_tbl / LIG + 2;
    constexpr int RL = 64;   // lanes per row
    rt.assign(rows * RL, make_uint4(0, 0, 0, 0));
    auto addr = [&](uint32_t slot, int grp) -> uint32_t { return 16u * (((slot & 64) ? 0 : SC + grp * SG) + (slot & 63)); };
    for (uint32_t pc = 0; pc * 4 + 3 < p.n_hdr; pc++) {
        const uint32_t h0 = p.hdr[4 * pc], off = p.hdr[4 * pc + 2];
        if ((h0 & 0xff) != OP_MULACC) continue;
        const uint32_t T = (h0 >> 8) & 0xff;
        for (int lane = 0; lane < RL; lane++) {
            const int g0 = lane / LIG, lig = lane - g0 * LIG, grp = g0 < GROUPS ? g0 : GROUPS - 1;
            uint32_t f1 = 0, f2 = 0;
            for (uint32_t t = 0; t < T; t++) {
                const uint32_t w = p.tbl[off + t * LIG + lig];
                rt[(off / LIG + t) * RL + lane] =
                    make_uint4(addr(w & 127, grp), addr((w >> 14) & 127, grp), addr((w >> 7) & 127, grp) | (addr((w >> 21) & 127, grp) << 16), 0);
                f1 |= ((w >> 30) & 1) << t | ((w >> 31) & 1) << (12 + t);
                f2 |= ((w >> 28) & 1) << t | ((w >> 29) & 1) << (12 + t);
            }
            // z, w: LDS byte address of the step's result slot / companion slot for this lane, -1 where it stores nothing
            // (a padding lane of the step, lanes 60..63 of a wavefront)
            const uint32_t ew = p.tbl[off + T * LIG + lig];
            const bool owner = g0 < GROUPS;
            const uint32_t dst = (owner && ((ew >> 7) & 1)) ? addr(ew & 63, grp) : 0xffffffffu;
            const uint32_t sd = (owner && ((ew >> 29) & 1)) ? addr((ew >> 23) & 63, grp) : 0xffffffffu;
            rt[(off / LIG + T) * RL + lane] = make_uint4(f1, f2, dst, sd);
        }
    }
}

hipError_t coop_init(CoopState* st, const hipDeviceProp_t& prop) {
    st->cus = prop.multiProcessorCount;
    CoopDev* d = new CoopDev();
    memset(d, 0, sizeof(*d));
    st->d_prog = d;          // coop_free releases whatever exists if the initialisation stops half way
    hipError_t e;
    for (int i = 0; i < ZKP_PROG_COUNT; i++) {
        const ZkpProgDesc& p = ZKP_PROGS[i];
        if ((e = hipMalloc((void**)&d->progs[i].hdr, p.n_hdr * 4)) != hipSuccess) return e;
        if ((e = hipMalloc((void**)&d->progs[i].tbl, (p.n_tbl + 2 * LIG + 4) * 4)) != hipSuccess) return e;
        if ((e = hipMemset(d->progs[i].tbl, 0, (p.n_tbl + 2 * LIG + 4) * 4)) != hipSuccess) return e;   // the kernel reads table words two terms ahead
        if ((e = hipMemcpy(d->progs[i].hdr, p.hdr, p.n_hdr * 4, hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(d->progs[i].tbl, p.tbl, p.n_tbl * 4, hipMemcpyHostToDevice)) != hipSuccess) return e;
        d->progs[i].nslot = p.nslot;
        d->progs[i].nconst = p.nconst;
        d->progs[i].wide = p.wide;
        std::vector<uint4> rt;
        coop_resolve_table(p, rt);
        if ((e = hipMalloc((void**)&d->progs[i].rtbl, rt.size() * sizeof(uint4))) != hipSuccess) return e;
        zkp_dbg_alloc("prog.hdr", d->progs[i].hdr, p.n_hdr * 4);
        zkp_dbg_alloc("prog.tbl", d->progs[i].tbl, (p.n_tbl + 2 * LIG + 4) * 4);
        zkp_dbg_alloc("prog.rtbl", d->progs[i].rtbl, rt.size() * sizeof(uint4));
        if ((e = hipMemcpy(d->progs[i].rtbl, rt.data(), rt.size() * sizeof(uint4), hipMemcpyHostToDevice)) != hipSuccess) return e;
    }
    if ((e = hipMalloc((void**)&d->consts, sizeof(ZKP_COOP_CONSTS))) != hipSuccess) return e;
    if ((e = hipMemcpy(d->consts, ZKP_COOP_CONSTS, sizeof(ZKP_COOP_CONSTS), hipMemcpyHostToDevice)) != hipSuccess) return e;
    // chunks of a batch are processed by n_pipes independent pipelines on separate HIP streams so that the
    // tail of one kernel (and the latency-bound inversion) overlaps the next chunk's work
    // every knob is read ONCE per context, here, and clamped by plan::clamp (zkp_plan.hpp): measured defaults - 2 pipes x 2^16 checks;
    // phase C in one launch sequence above one chunk (2^17 / 2^18 / 2^19 checks: 37.1 / 72.9 / 142.4 ms against 37.6 / 73.6 / 142.9 per
    // chunk), in two parts on the pipelines from 2^18 checks on; inversion: half a wavefront per SIMD runs its chain fastest
    auto env_l = [](const char* name, long dflt) -> long { const char* v = getenv(name); return v ? atol(v) : dflt; };
    plan::Knobs kn;
    kn.n_pipes = (int)env_l("ZKP_COOP_STREAMS", kn.n_pipes);
    kn.chunk = (size_t)env_l("ZKP_COOP_CHUNK", (long)kn.chunk);
    kn.super = (size_t)env_l("ZKP_COOP_SUPER", (long)kn.super);
    kn.inv_batch = (uint32_t)env_l("ZKP_COOP_INV_BATCH", (long)kn.inv_batch);
    kn.inv_lanes = (size_t)env_l("ZKP_COOP_INV_LANES", (long)kn.inv_lanes);
    // ZKP_COOP_NO_STREAM=1: groups of eight pairs joined by f12mul, the flow of rounds 1-4 (A/B baseline, cross-check);
    // ZKP_COOP_MAX_STREAM: pairs per streamed group, 9 .. 64 (sweeps)
    const long ms_env = env_l("ZKP_COOP_MAX_STREAM", 0);
    kn.max_stream = env_l("ZKP_COOP_NO_STREAM", 0) != 0 ? plan::MAX_GROUP
                    : (ms_env > (long)plan::MAX_GROUP && ms_env <= (long)plan::MAX_STREAM_LIMIT ? (size_t)ms_env : plan::MAX_STREAM);
    kn.c_split = (int)env_l("ZKP_COOP_C_SPLIT", 0);
    kn.c_split_min = (size_t)env_l("ZKP_COOP_C_SPLIT_MIN", (long)kn.c_split_min);
    kn.split_min = (size_t)env_l("ZKP_COOP_SPLIT_MIN", (long)kn.split_min);
    d->kn = plan::clamp(kn);
    d->inv_fermat = env_l("ZKP_COOP_INV_FERMAT", 0) != 0;
    d->cus = prop.multiProcessorCount;
    d->prime = (int)env_l("ZKP_COOP_PRIME", 1);
    d->miller1 = env_l("ZKP_COOP_MILLER1", 1) != 0;
    for (int i = 0; i < MAX_PIPES; i++) d->pipe[i].owner = d;
    for (int i = 0; i < d->kn.n_pipes; i++) {
        if ((e = hipStreamCreateWithFlags(&d->pipe[i].stream, hipStreamNonBlocking)) != hipSuccess) return e;
        if ((e = hipEventCreateWithFlags(&d->pipe[i].done, hipEventDisableTiming)) != hipSuccess) return e;
    }
    if ((e = hipEventCreateWithFlags(&d->ready, hipEventDisableTiming)) != hipSuccess) return e;
    st->available = true;
    return hipSuccess;
}

void coop_free(CoopState* st) {
    CoopDev* d = (CoopDev*)st->d_prog;
    if (!d) return;
    for (int i = 0; i < ZKP_PROG_COUNT; i++) {
        if (d->progs[i].hdr) (void)hipFree(d->progs[i].hdr);
        if (d->progs[i].tbl) (void)hipFree(d->progs[i].tbl);
        if (d->progs[i].rtbl) (void)hipFree(d->progs[i].rtbl);
    }
    if (d->consts) (void)hipFree(d->consts);
    if (d->big_state) (void)hipFree(d->big_state);
    if (d->vscratch) (void)hipFree(d->vscratch);
    for (int i = 0; i < MAX_PIPES; i++) {
        if (d->pipe[i].lines) (void)hipFree(d->pipe[i].lines);
        if (d->pipe[i].state) (void)hipFree(d->pipe[i].state);
        if (d->pipe[i].stream) (void)hipStreamDestroy(d->pipe[i].stream);
        if (d->pipe[i].done) (void)hipEventDestroy(d->pipe[i].done);
    }
    if (d->ready) (void)hipEventDestroy(d->ready);
    delete d;
    st->d_prog = nullptr;
    st->available = false;
}

// AUTO (0) and COOP (2) route through this family; THREAD (1) forces the one-pairing-per-lane kernels
bool coop_selected(const CoopState* st, int kind) { return st->available && kind != 1; }

static hipError_t ensure_buf(int4** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return hipSuccess;
    if (*p) { hipError_t e = hipFree(*p); if (e != hipSuccess) return e; *p = nullptr; *cap = 0; }
    hipError_t e = hipMalloc((void**)p, bytes);
    if (e == hipSuccess) { *cap = bytes; zkp_dbg_alloc("coop.buf", *p, bytes); }
    return e;
}

// Round 6: where the wavefronts of a SMALL grid land depends on what the dispatcher placed last.  On an idle GPU, or behind a kernel of
// another shape, 1,024 one-wavefront workgroups (one per SIMD if spread evenly) come to lie two to a SIMD on half of the SIMDs and take as
// long as 1,536 (k_ksq: 375 us where 768 wavefronts take 220); 2,048 come to lie three to a SIMD (550 us where 1,536 take 385).  Behind a
// grid of the SAME size they spread evenly - even when that grid is an empty kernel (tools/occupancy_probe.py, profiles/r06/placement_probe.txt).
// So a launch whose grid falls into a bad band is preceded by a PRIMER: an empty kernel on the same grid (3-4 us).  The bands, measured per
// kernel class (profiles/r06/knob_sweeps.txt r6o, r6p): k_ksq more than 3 and at most 4, or more than 6 and at most 8 workgroups per compute
// unit (16,384 / 32,768 checks: 6.5 -> 5.8 / 10.4 -> 9.6 ms per pass); k_prep_lines and k_batch_inv more than 2 and at most 3 (20,480 /
// 24,576 pairs: 7.5 -> 6.8 / 8.3 -> 7.5 ms); the interpreter's and the decompression's launches gain nothing and are not primed.  Only
// batches of at most one chunk are primed (a larger one keeps the GPU full).  LDS padding to cap the workgroups per
// compute unit does nothing here (the imbalance is between the SIMDs of a compute unit).  ZKP_COOP_PRIME: 0 off, 1 the bands (default),
// 2 every grid of 1 .. 12 workgroups per compute unit of the primed classes.
static hipError_t prime(const CoopDev* d, hipStream_t s, size_t blocks, int cls) {
    if (!d || !d->prime || d->cus <= 0 || !blocks || !d->prime_now) return hipSuccess;
    const size_t c = (size_t)d->cus;
    const bool band = cls == PRIME_KSQ ? (blocks > 3 * c && blocks <= 4 * c) || (blocks > 6 * c && blocks <= 8 * c)      // three wavefronts per SIMD
                                       : (blocks > 2 * c && blocks <= 3 * c);
    if (!(band || (d->prime >= 2 && blocks > c && blocks <= 12 * c))) return hipSuccess;
    hipLaunchKernelGGL(k_primer, dim3((unsigned)blocks), dim3(64), 0, s);
    return hipGetLastError();
}

static hipError_t run_prog(CoopDev* d, CoopPipe* pp, int prog, uint32_t n_checks, uint32_t nc, uint32_t k, const uint64_t* wire_in,
                           uint64_t* wire_out, uint8_t* ok, int* all_ok, uint32_t st_off = 0, uint32_t chk_off = 0, bool miller1 = false) {
    hipStream_t s = pp->stream;
    CoopArgs a;
    a.hdr = d->progs[prog].hdr;
    a.tbl = d->progs[prog].tbl;
    a.rtbl = d->progs[prog].rtbl;
    a.consts = d->consts;
    a.lines = pp->lines;
    a.state = pp->state;
    a.wire_in = wire_in;
    a.wire_out = wire_out;
    a.ok = ok;
    a.all_ok = all_ok;
    a.n_checks = n_checks;
    a.nc = nc;
    a.k = k;
    const uint32_t cfg = d->progs[prog].wide;      // LDS configuration: 0 plain, 1 wide, 2 deep (tools/coopgen.py lds_config)
    if (cfg > 2 || d->progs[prog].nslot > (uint32_t)coop_cfg_slots(cfg) || d->progs[prog].nconst > (uint32_t)coop_cfg_consts(cfg))
        return hipErrorInvalidValue;
    a.S = coop_cfg_slots(cfg);
    a.nconst = d->progs[prog].nconst;
    a.st_off = st_off;
    a.chk_off = chk_off;
    a.nd = pp->nd;

    static_assert(12 * coop_lds_bytes(ZKP_COOP_NSLOT, ZKP_COOP_NCONST) <= 160 * 1024 &&
                      12 * coop_lds_bytes(ZKP_COOP_WIDE_NSLOT, ZKP_COOP_WIDE_NCONST) <= 160 * 1024 &&
                      12 * coop_lds_bytes(ZKP_COOP_DEEP_NSLOT, ZKP_COOP_DEEP_NCONST) <= 160 * 1024,
                  "twelve wavefronts (three per SIMD, the register bound) must fit the 160 KB of LDS of a CU");
    const size_t lds_bytes = coop_lds_bytes(coop_cfg_slots(cfg), coop_cfg_consts(cfg));
    unsigned blocks = (n_checks + GROUPS - 1) / GROUPS;
    ProfScope prof(d, s, cfg == 1 ? PROF_MILLER : cfg == 2 ? PROF_C_DEEP : d->prof_phase_c ? PROF_C_PLAIN : PROF_FEXP_A);
    if (miller1) {   // the program's own kernel: same image, same arguments (k_miller1 addresses lines and state with 32-bit byte offsets)
        if (prog != ZKP_PROG_MILLER1_STATE || cfg != 1 || !zkp::m1::eligible(n_checks, nc, st_off))
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_miller1, dim3(blocks), dim3(64), lds_bytes, s, a);
    } else if (cfg == 2)
        hipLaunchKernelGGL((k_coop<ZKP_COOP_DEEP_NSLOT, ZKP_COOP_DEEP_NCONST>), dim3(blocks), dim3(64), lds_bytes, s, a);
    else if (cfg == 1)
        hipLaunchKernelGGL((k_coop<ZKP_COOP_WIDE_NSLOT, ZKP_COOP_WIDE_NCONST>), dim3(blocks), dim3(64), lds_bytes, s, a);
    else
        hipLaunchKernelGGL((k_coop<ZKP_COOP_NSLOT, ZKP_COOP_NCONST>), dim3(blocks), dim3(64), lds_bytes, s, a);
    return hipGetLastError();
}

static int miller_prog(size_t k, bool wire) {
    switch (k) {
        case 1: return wire ? ZKP_PROG_MILLER1_WIRE : ZKP_PROG_MILLER1_STATE;
        case 2: return wire ? ZKP_PROG_MILLER2_WIRE : ZKP_PROG_MILLER2_STATE;
        case 3: return wire ? ZKP_PROG_MILLER3_WIRE : ZKP_PROG_MILLER3_STATE;
        case 4: return wire ? ZKP_PROG_MILLER4_WIRE : ZKP_PROG_MILLER4_STATE;
        case 5: return wire ? ZKP_PROG_MILLER5_WIRE : ZKP_PROG_MILLER5_STATE;
        case 6: return wire ? ZKP_PROG_MILLER6_WIRE : ZKP_PROG_MILLER6_STATE;
        case 7: return wire ? ZKP_PROG_MILLER7_WIRE : ZKP_PROG_MILLER7_STATE;
        case 8: return wire ? ZKP_PROG_MILLER8_WIRE : ZKP_PROG_MILLER8_STATE;
        default: return -1;
    }
}

constexpr size_t MAX_GROUP = plan::MAX_GROUP;   // pairs per UNROLLED Miller program (miller1..8)
// round 5: more pairs run through the run-time-k program (millern: a pair loop inside every iteration, ONE accumulator, the 63 squarings
// shared by all of them) in groups of at most kn.max_stream pairs; a check with more pairs is joined from its groups' Miller values by
// f12mul as before.  16 is the measured optimum (multi_miller_loop() of 2^20 / 2^18 pairs in checks of k, same box, ms; groups of 8 |
// 16 | 64): k = 9: 89.4 | 85.9 | 84.5, 12: 90.6 | 87.9 | 86.7, 16: 85.6 | 87.8 | 85.9, 32: 93.1 | 86.1 | 93.9, 48: 105.0 | 93.6 | 113.1,
// 64: 107.6 | 102.7 | 116.3, 96: 114.6 | 110.4 | 141.0 (2^18 pairs: 9: 26.5 | 23.0 | 23.3, 16: 27.0 | 25.8 | 25.8, 64: 36.0 | 33.9 | 41.3) -
// longer groups shrink the chunks the line buffer allows (26 KB per pair) until a launch no longer fills the GPU
bool coop_supports_k(size_t k) { return k >= 1 && k <= 0xffffu; }

// line stream of pairs j0 .. j0+g-1 of each of the n checks starting at base_check (k_in pairs per check)
// fused: the Miller value only feeds a final exponentiation inside the same call (homogeneous projective steps, freely scaled lines)
static hipError_t prep(CoopPipe* pp, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t base_check, uint32_t n,
                       uint32_t k_in, uint32_t j0, uint32_t g, bool fused) {
    hipStream_t s = pp->stream;
    size_t p0 = base_check * k_in;
    uint32_t n_pairs = n * g;
    const size_t prep_lds = 4 * 4 * 64 * sizeof(int4);
    { hipError_t ep = prime(pp->owner, s, (2 * (size_t)n_pairs + 63) / 64, PRIME_PREP); if (ep != hipSuccess) return ep; }
    ProfScope prof(pp->owner, s, PROF_PREP);
    if (fused) {   // the CLN steps, then the Jacobian steps for the wavefronts with a G2 point off the twist (normally none: they return)
        hipLaunchKernelGGL(k_prep_lines<true>, dim3((2 * n_pairs + 63) / 64), dim3(64), prep_lds, s, g1 + 12 * p0, g2 + 24 * p0,
                           i1 ? i1 + p0 : nullptr, i2 ? i2 + p0 : nullptr, n_pairs, g, k_in, j0, n, pp->lines, pp->nd);
        hipLaunchKernelGGL(k_prep_lines_off_twist, dim3((2 * n_pairs + 63) / 64), dim3(64), prep_lds, s, g1 + 12 * p0, g2 + 24 * p0,
                           i1 ? i1 + p0 : nullptr, i2 ? i2 + p0 : nullptr, n_pairs, g, k_in, j0, n, pp->lines, pp->nd);
    } else
        hipLaunchKernelGGL(k_prep_lines<false>, dim3((2 * n_pairs + 63) / 64), dim3(64), prep_lds, s, g1 + 12 * p0, g2 + 24 * p0, i1 ? i1 + p0 : nullptr,
                           i2 ? i2 + p0 : nullptr, n_pairs, g, k_in, j0, n, pp->lines, pp->nd);
    return hipGetLastError();
}

// multi_miller_loop of n checks of k pairs each on one pipeline.  k <= 8: one program.  k > 8: groups of at most
// eight pairs run their own Miller loop (the line buffer is reused), the group values are joined by f12mul
// (prod_i f_i is the multi-Miller value; only the shared squarings are lost).  Result: state ST_F, or the
// canonical wire record in `wire_out` when that is not null.
static hipError_t miller_on_pipe(CoopDev* d, CoopPipe* pp, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2,
                                 size_t base, uint32_t n, uint32_t nc, size_t k, uint64_t* wire_out, bool fused = false) {
    hipError_t e;
    if (k <= MAX_GROUP) {
        if ((e = prep(pp, g1, g2, i1, i2, base, n, (uint32_t)k, 0, (uint32_t)k, fused)) != hipSuccess) return e;
        // one pair per check, result in the state record (the fused pairing path): k_miller1, unless the knob or the 32-bit byte
        // offsets of that kernel (a line buffer, or the twelve Miller elements of a state buffer, beyond 4 GB) say the interpreter
        const bool m1 = d->miller1 && k == 1 && !wire_out && zkp::m1::eligible(n, nc, 0);
        return run_prog(d, pp, miller_prog(k, wire_out != nullptr), n, nc, (uint32_t)k, nullptr, wire_out, nullptr, nullptr, 0, 0, m1);
    }
    const size_t MS = d->kn.max_stream;
    if (k <= MS) {               // one accumulator for all k pairs
        if ((e = prep(pp, g1, g2, i1, i2, base, n, (uint32_t)k, 0, (uint32_t)k, fused)) != hipSuccess) return e;
        return run_prog(d, pp, wire_out ? ZKP_PROG_MILLERN_WIRE : ZKP_PROG_MILLERN_STATE, n, nc, (uint32_t)k, nullptr, wire_out, nullptr, nullptr);
    }
    for (size_t j0 = 0; j0 < k; j0 += MS) {
        const size_t g = k - j0 < MS ? k - j0 : MS;
        if ((e = prep(pp, g1, g2, i1, i2, base, n, (uint32_t)k, (uint32_t)j0, (uint32_t)g, fused)) != hipSuccess) return e;
        if ((e = run_prog(d, pp, g <= MAX_GROUP ? miller_prog(g, false) : ZKP_PROG_MILLERN_STATE, n, nc, (uint32_t)g, nullptr, nullptr, nullptr, nullptr,
                          j0 ? ZKP_COOP_ST_G : 0)) != hipSuccess)
            return e;
        if (j0) {
            const bool last = j0 + g == k;
            if ((e = run_prog(d, pp, (last && wire_out) ? ZKP_PROG_F12MUL_WIRE : ZKP_PROG_F12MUL_STATE, n, nc, 1, nullptr, last ? wire_out : nullptr,
                              nullptr, nullptr)) != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

// Run `body(pipe, base, n)` for every chunk of the batch, round-robin over the pipelines.  The caller's
// stream `s` is forked into the pipeline streams (they wait for everything already queued on `s`) and
// joined again at the end, so from the caller's point of view the call is ordered on `s`.
template <class Body>
static hipError_t for_chunks(CoopDev* d, size_t n_total, size_t k, bool need_lines, bool need_state, hipStream_t s, Body body, size_t chunk_override = 0) {
    if (!n_total) return hipSuccess;
    hipError_t e;
    const plan::Chunks pc = plan::plan_chunks(d->kn, n_total, k, need_lines, chunk_override, d->prof != nullptr);
    const size_t chunk = pc.chunk;
    const int pipes = pc.pipes;
    // workspace first: hipMalloc/hipFree synchronise the device, so never (re)allocate between launches
    for (int i = 0; i < pipes; i++) {
        if (need_lines && (e = ensure_buf(&d->pipe[i].lines, &d->pipe[i].lines_bytes, plan::lines_bytes(plan::group_size(d->kn, k), pc.cmax))) != hipSuccess) return e;
        if (need_state && (e = ensure_buf(&d->pipe[i].state, &d->pipe[i].state_bytes, plan::state_bytes(pc.cmax))) != hipSuccess) return e;
    }
    if ((e = hipEventRecord(d->ready, s)) != hipSuccess) return e;
    for (int i = 0; i < pipes; i++)
        if ((e = hipStreamWaitEvent(d->pipe[i].stream, d->ready, 0)) != hipSuccess) return e;
    int c = 0;
    for (size_t base = 0; base < n_total; base += chunk, c++) {
        uint32_t n = (uint32_t)((n_total - base) < chunk ? (n_total - base) : chunk);
        if ((e = body(&d->pipe[c % pipes], base, n)) != hipSuccess) return e;
    }
    for (int i = 0; i < pipes; i++) {
        if ((e = hipEventRecord(d->pipe[i].done, d->pipe[i].stream)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(s, d->pipe[i].done, 0)) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t coop_miller(CoopState* st, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n_checks, size_t k,
                       uint64_t* out, hipStream_t s) {
    CoopDev* d = (CoopDev*)st->d_prog;
    if (!coop_supports_k(k)) return hipErrorNotSupported;
    d->prime_now = n_checks <= d->kn.chunk;
    return for_chunks(d, n_checks, k, true, true, s, [&](CoopPipe* pp, size_t base, uint32_t n) -> hipError_t {
        return miller_on_pipe(d, pp, g1, g2, i1, i2, base, n, n, k, out + 72 * base);
    });
}

// nsq compressed squarings of the Fp12 value in state elements [elem_in, elem_in + 12) of every check, snapshots of
// (z2..z5) after the squarings whose bit is set in snap_mask into 12-element areas from elem_snap on
static hipError_t run_ksq(hipStream_t s, int4* state, uint32_t n_checks, uint32_t nc, uint32_t elem_in, uint32_t elem_snap, uint32_t nsq,
                          uint64_t snap_mask, CoopDev* d = nullptr, NDev nd = NDev{nullptr, 0}) {
    if (!n_checks || !nsq) return hipSuccess;
    if (snap_mask && nsq > 64) return hipErrorInvalidValue;   // snapshot bits exist for the first 64 squarings only
    { hipError_t ep = prime(d, s, (n_checks + KS_CHECKS - 1) / KS_CHECKS, PRIME_KSQ); if (ep != hipSuccess) return ep; }
    ProfScope prof(d, s, PROF_KSQ);
    hipLaunchKernelGGL(k_ksq, dim3((n_checks + KS_CHECKS - 1) / KS_CHECKS), dim3(64), 7 * 64 * sizeof(int4), s, state, n_checks, nc, elem_in, elem_snap, nsq, snap_mask, nd);
    return hipGetLastError();
}

// batched inversion of `count` planes of n per-check values (k_batch_inv): few lanes with long batches, because the kernel
// is bound by the latency of one lane's chain (610 + 3 B multiplications)
static hipError_t run_inv(CoopDev* d, hipStream_t s, int4* state, uint32_t n, uint32_t nc, uint32_t elem_n, uint32_t elem_ninv, uint32_t count,
                          NDev nd = NDev{nullptr, 0}) {
    const size_t total = (size_t)n * count;
    if (!total) return hipSuccess;
    const plan::Inv pi = plan::plan_inv(d->kn, n, count);
    const uint32_t B = pi.batch;
    const size_t lanes = pi.lanes;
    { hipError_t ep = prime(d, s, (lanes + 63) / 64, PRIME_INV); if (ep != hipSuccess) return ep; }
    ProfScope prof(d, s, PROF_INV);
    hipLaunchKernelGGL(k_batch_inv, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, state, n, nc, B | (d->inv_fermat ? 0x80000000u : 0u), elem_n,
                       elem_ninv, count, nd);
    return hipGetLastError();
}

// phase C of the final exponentiation: the generated plan (tools/coopgen.py prog_fexp_c) alternates step programs of the
// interpreter with the compressed squaring runs of the five x-power chains and the decompression of their snapshots.
// Everything runs on pp->stream over the n checks whose state starts at pp->state (record stride nc).
static hipError_t run_fexp_c(CoopDev* d, CoopPipe* pp, uint32_t n, uint32_t nc, uint64_t* wire_out, uint8_t* ok, int* all_ok) {
    hipError_t e;
    d->prof_phase_c = true;
    for (int i = 0; i < ZKP_FEXP_C_PLAN_LEN; i++) {
        const ZkpPlanStep& ps = ZKP_FEXP_C_PLAN[i];
        switch (ps.kind) {
            case ZKP_PLAN_PROG:
                e = run_prog(d, pp, (int)ps.a, n, nc, 1, nullptr, wire_out, ok, all_ok);
                break;
            case ZKP_PLAN_KSQ:
                e = run_ksq(pp->stream, pp->state, n, nc, ps.a, ps.b, ps.c, ps.mask, d, pp->nd);
                break;
            case ZKP_PLAN_KDEC_A: {
            ProfScope prof(d, pp->stream, PROF_KDEC_A);
                hipLaunchKernelGGL(k_kdec_a, dim3((unsigned)((2 * (size_t)n * ps.b + 63) / 64)), dim3(64), 0, pp->stream, pp->state, n, nc, ps.a, ps.b, ps.c, pp->nd);
                e = hipGetLastError();
                break;
            }
            case ZKP_PLAN_INV:
                e = run_inv(d, pp->stream, pp->state, n, nc, ps.a, ps.b, ps.c, pp->nd);
                break;
            case ZKP_PLAN_KDEC_B: {
            ProfScope prof(d, pp->stream, PROF_KDEC_B);
                hipLaunchKernelGGL(k_kdec_b, dim3((unsigned)((2 * (size_t)n * ps.b + 63) / 64)), dim3(64), 0, pp->stream, pp->state, n, nc, ps.a, ps.b, ps.c, pp->nd);
                e = hipGetLastError();
                break;
            }
            default:
                e = hipErrorInvalidValue;
        }
        if (e != hipSuccess) break;
    }
    d->prof_phase_c = false;
    return e;
}

// Final exponentiation in two phases over a super-chunk of checks that share ONE state buffer: phase A per chunk on
// the pipelines (whatever produces ST_F, then fexp_a down to the single Fp inversion), ONE batched inversion over all
// checks of the super-chunk (k_batch_inv is latency bound: per 2^16-check chunk it would leave the GPU idle for ~1.5 ms),
// phase C (fexp_c) per chunk.
template <class PhaseA>
static hipError_t two_phase(CoopDev* d, size_t n_total, size_t k, bool need_lines, hipStream_t s, uint64_t* out, uint8_t* ok, int* all_ok,
                            PhaseA phase_a) {
    hipError_t e;
    for (size_t sb = 0; sb < n_total; sb += d->kn.super) {
        const size_t ns = n_total - sb < d->kn.super ? n_total - sb : d->kn.super;
        d->prime_now = ns <= d->kn.chunk && n_total <= d->kn.chunk;
        if ((e = ensure_buf(&d->big_state, &d->big_state_bytes, plan::state_bytes(ns))) != hipSuccess) return e;
        e = for_chunks(d, ns, k, need_lines, false, s, [&](CoopPipe* pp, size_t base, uint32_t n) -> hipError_t {
            CoopPipe v = *pp;
            v.state = d->big_state + 4 * base;
            v.nd = NDev{d->n_dev, (uint32_t)(sb + base)};
            return phase_a(&v, sb + base, n, (uint32_t)ns);
        });
        if (e != hipSuccess) return e;
        if ((e = run_inv(d, s, d->big_state, (uint32_t)ns, (uint32_t)ns, ZKP_COOP_ST_N, ZKP_COOP_ST_NINV, 1, NDev{d->n_dev, (uint32_t)sb})) != hipSuccess) return e;
        // phase C needs no line buffer.  The plan (zkp_plan.hpp plan_phase_c): two parts on the two pipelines from 2^18 checks on (round 5,
        // same-box A/B one sequence -> two parts: 2^20 234.1 / 236.0 -> 233.4 / 233.4 ms; 2^19 117.7 / 117.5 -> 115.1 / 114.8; 2^18 60.2 /
        // 60.1 -> 59.1 / 58.6; 2^17 a wash), ONE launch sequence on the caller's stream below.  Round 6 measured the small and medium
        // batches (profiles/r06/knob_sweeps.txt, the v60 traces beside it): what a 2^16 / 2^17-check batch loses against the 2^20 rate is
        // the six k_batch_inv launches - 0.11-0.18 ms each whatever the batch, one lane's dependent chain - and the round quantisation of
        // k_ksq (4,096 / 8,192 wavefronts on 3,072 slots).  Two parts at these sizes lose (2^16: 16.4 -> 17.1 ms) - each half-size launch
        // has its own partial round - and two parts kept OUT of phase by events (the follower's squaring run c starts when the leader's
        // has ended, so that one part's inversion runs beside the other's squaring run) hide the inversion but not for free: beside a
        // squaring run it takes 0.44 instead of 0.13 ms and the run 7 % longer; 16.6 / 31.5 ms against 16.4 / 31.5.  More inversion
        // lanes, an occupancy cap and chunks of 2^13 .. 2^15 all lose as well.  ZKP_COOP_C_SPLIT=n forces n parts (A/B, tests).
        const plan::PhaseC pcc = plan::plan_phase_c(d->kn, ns, d->prof != nullptr);
        if (pcc.mode == plan::C_PARTS) {
            const size_t part = pcc.part;
            e = for_chunks(d, ns, 1, false, false, s, [&](CoopPipe* pp, size_t base, uint32_t n) -> hipError_t {
                CoopPipe v = *pp;
                v.state = d->big_state + 4 * base;
                v.nd = NDev{d->n_dev, (uint32_t)(sb + base)};
                return run_fexp_c(d, &v, n, (uint32_t)ns, out ? out + 72 * (sb + base) : nullptr, ok ? ok + sb + base : nullptr, all_ok);
            }, part);
        } else {
            CoopPipe v = d->pipe[0];
            v.state = d->big_state;
            v.stream = s;
            v.nd = NDev{d->n_dev, (uint32_t)sb};
            e = run_fexp_c(d, &v, (uint32_t)ns, (uint32_t)ns, out ? out + 72 * sb : nullptr, ok ? ok + sb : nullptr, all_ok);
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t coop_final_exp(CoopState* st, const uint64_t* f, size_t n_total, uint64_t* out, uint8_t* ok, int* all_ok, hipStream_t s) {
    CoopDev* d = (CoopDev*)st->d_prog;
    return two_phase(d, n_total, 1, false, s, out, ok, all_ok, [&](CoopPipe* pp, size_t base, uint32_t n, uint32_t nc) -> hipError_t {
        return run_prog(d, pp, ZKP_PROG_FEXP_A_WIRE, n, nc, 1, f + 72 * base, nullptr, nullptr, nullptr);
    });
}

// one level of the Fp12 product tree, in place: buf[c] <- buf[c] * buf[c + h] for c < m  (m <= h)
hipError_t coop_fp12_mul_pairs(CoopState* st, uint64_t* buf, size_t m, size_t h, hipStream_t s) {
    CoopDev* d = (CoopDev*)st->d_prog;
    if (m > 0xffffffffu || h > 0xffffffffu) return hipErrorInvalidValue;
    CoopPipe on_s = d->pipe[0];   // no workspace is touched: only the stream matters
    on_s.stream = s;
    return run_prog(d, &on_s, ZKP_PROG_F12MUL_PAIRS, (uint32_t)m, (uint32_t)m, 1, buf, buf, nullptr, nullptr, 0, (uint32_t)h);
}

hipError_t coop_pairing(CoopState* st, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n_checks, size_t k,
                        uint64_t* out_gt, uint8_t* ok, int* all_ok, hipStream_t s, const uint32_t* n_dev) {
    CoopDev* d = (CoopDev*)st->d_prog;
    if (!coop_supports_k(k)) return hipErrorNotSupported;
    // n_dev (device memory, may be null): only the first min(n_checks, *n_dev) checks exist - the launches are planned for n_checks and
    // size themselves on the device (NDev); nothing is read back
    d->n_dev = n_dev;
    const hipError_t e2 = two_phase(d, n_checks, k, true, s, out_gt, ok, all_ok, [&](CoopPipe* pp, size_t base, uint32_t n, uint32_t nc) -> hipError_t {
        hipError_t e = miller_on_pipe(d, pp, g1, g2, i1, i2, base, n, nc, k, nullptr, true);
        if (e != hipSuccess) return e;
        return run_prog(d, pp, ZKP_PROG_FEXP_A_STATE, n, nc, 1, nullptr, nullptr, nullptr, nullptr);
    });
    d->n_dev = nullptr;
    return e2;
}

// one pass of the fused pairing with every launch bracketed by events (one pipeline: no two kernels overlap); ms[c] = the
// summed duration of the launches of class c, launches[c] their number.  Synchronises `s`.
hipError_t coop_profile_pairing(CoopState* st, const uint64_t* g1, const uint64_t* g2, size_t n, uint64_t* out_gt, float* ms, int* launches, hipStream_t s) {
    CoopDev* d = (CoopDev*)st->d_prog;
    std::vector<CoopDev::ProfEv> evs;
    struct ProfGuard {       // d->prof points at this frame's vector: it is taken back on EVERY way out (push_back may throw)
        CoopDev* d;
        ~ProfGuard() { d->prof = nullptr; d->prof_phase_c = false; }
    } guard{d};
    d->prof = &evs;
    hipError_t e;
    try {
        e = coop_pairing(st, g1, g2, nullptr, nullptr, n, 1, out_gt, nullptr, nullptr, s, nullptr);
    } catch (...) {
        e = hipErrorOutOfMemory;
    }
    d->prof = nullptr;
    d->prof_phase_c = false;
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    for (int c = 0; c < PROF_CLASSES; c++) { ms[c] = 0.f; launches[c] = 0; }
    for (auto& ev : evs) {
        float t = 0.f;
        if (e == hipSuccess && (e = hipEventElapsedTime(&t, ev.a, ev.b)) == hipSuccess) { ms[ev.cls] += t; launches[ev.cls]++; }
        (void)hipEventDestroy(ev.a);
        (void)hipEventDestroy(ev.b);
    }
    return e;
}

// zkp_tower_op_batch on the cooperative family: `ab` holds the n a-records followed by the n b-records (wire format);
// op as in zkp_tower_op (include/zkp_pairings.h).  The cyclotomic power g^(2^repeat) (and the decompression alone) takes the route of the final
// exponentiation's x-power chains: wire -> state, one compressed squaring run with a single snapshot, decompression, -> wire.
hipError_t coop_tower_op(CoopState* st, int op, const uint64_t* ab, size_t n, uint32_t repeat, uint64_t* out, hipStream_t s) {
    CoopDev* d = (CoopDev*)st->d_prog;
    static const int progs[11] = {ZKP_PROG_TW_FP2_MUL, ZKP_PROG_TW_FP2_SQR, ZKP_PROG_TW_FP6_MUL, ZKP_PROG_TW_FP6_SQR, ZKP_PROG_TW_FP12_FROB,
                                  ZKP_PROG_TW_FP12_MUL, ZKP_PROG_TW_FP12_SQR, ZKP_PROG_TW_FP12_014, ZKP_PROG_TW_FP12_FROB, ZKP_PROG_TW_FP12_CONJ,
                                  ZKP_PROG_TW_CYC_SQR};
    if (op < 0 || op > 20 || n > 0x3fffffffu) return hipErrorInvalidValue;
    d->prime_now = n <= d->kn.chunk;
    hipError_t e;
    for (size_t base = 0; base < n; base += d->kn.chunk) {
        const uint32_t m = (uint32_t)(n - base < d->kn.chunk ? n - base : d->kn.chunk);
        CoopPipe v = d->pipe[0];
        v.stream = s;
        if (op >= 13) {
            // round 4: the remaining tower functions of SURVEY 8(a).  One program for the sparse products and the nonresidue maps;
            // an inversion is program A (wire -> state, the norm chain down to ONE Fp value), the batched inversion kernel (0 gives
            // 0: a non-invertible input ends as the zero record), program B (state -> wire) - for Fp12 exactly the route
            // final_exponentiation() takes (fexp_a, k_batch_inv, the opening of fexp_c)
            int one = -1, pa = -1, pb = -1;
            switch (op) {
                case 13: pa = ZKP_PROG_TW_FP2_INV_A; pb = ZKP_PROG_TW_FP2_INV_B; break;
                case 14: one = ZKP_PROG_TW_FP2_NR; break;
                case 15: one = ZKP_PROG_TW_FP2_MULFP; break;
                case 16: one = ZKP_PROG_TW_FP6_BY1; break;
                case 17: one = ZKP_PROG_TW_FP6_BY01; break;
                case 18: one = ZKP_PROG_TW_FP6_NR; break;
                case 19: pa = ZKP_PROG_TW_FP6_INV_A; pb = ZKP_PROG_TW_FP6_INV_B; break;
                default: pa = ZKP_PROG_FEXP_A_WIRE; pb = ZKP_PROG_TW_FP12_INV_B; break;
            }
            if (one >= 0) {
                if ((e = run_prog(d, &v, one, m, m, 1, ab + 72 * base, out + 72 * base, nullptr, nullptr, 0, (uint32_t)n)) != hipSuccess) return e;
                continue;
            }
            if ((e = ensure_buf(&d->pipe[0].state, &d->pipe[0].state_bytes, plan::state_bytes(d->kn.chunk))) != hipSuccess) return e;
            v.state = d->pipe[0].state;
            if ((e = run_prog(d, &v, pa, m, m, 1, ab + 72 * base, nullptr, nullptr, nullptr)) != hipSuccess) return e;
            if ((e = run_inv(d, s, v.state, m, m, ZKP_COOP_ST_N, ZKP_COOP_ST_NINV, 1)) != hipSuccess) return e;
            if ((e = run_prog(d, &v, pb, m, m, 1, nullptr, out + 72 * base, nullptr, nullptr)) != hipSuccess) return e;
            continue;
        }
        if (op <= 10) {
            if ((e = run_prog(d, &v, progs[op], m, m, 1, ab + 72 * base, out + 72 * base, nullptr, nullptr, 0, (uint32_t)n)) != hipSuccess) return e;
            // ZKP_TOWER_FP6_FROBENIUS runs the Fp12 program; the Fp6 result is its c0 half, the rest of the record is zero whatever
            // the input's tail held (as the thread family's k_tower_op writes it)
            if (op == 4 && (e = hipMemset2DAsync(out + 72 * base + 36, 576, 0, 288, m, s)) != hipSuccess) return e;
            continue;
        }
        if (op == 11 && (repeat < 1 || repeat > 64)) return hipErrorInvalidValue;
        if ((e = ensure_buf(&d->pipe[0].state, &d->pipe[0].state_bytes, plan::state_bytes(d->kn.chunk))) != hipSuccess) return e;
        v.state = d->pipe[0].state;
        if (op == 12) {      // decompression alone: the record's z2..z5 are the snapshot
            if ((e = run_prog(d, &v, ZKP_PROG_TW_TO_SNAP, m, m, 1, ab + 72 * base, nullptr, nullptr, nullptr)) != hipSuccess) return e;
        } else {
            if ((e = run_prog(d, &v, ZKP_PROG_TW_TO_STATE, m, m, 1, ab + 72 * base, nullptr, nullptr, nullptr)) != hipSuccess) return e;
            if ((e = run_ksq(s, v.state, m, m, 0, ZKP_COOP_ST_SNAP, repeat, 1ull << (repeat - 1), d)) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_kdec_a, dim3((2 * m + 63) / 64), dim3(64), 0, s, v.state, m, m, (uint32_t)ZKP_COOP_ST_SNAP, 1u, (uint32_t)ZKP_COOP_ST_KN, NDev{nullptr, 0});
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = run_inv(d, s, v.state, m, m, ZKP_COOP_ST_KN, ZKP_COOP_ST_KNINV, 1)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_kdec_b, dim3((2 * m + 63) / 64), dim3(64), 0, s, v.state, m, m, (uint32_t)ZKP_COOP_ST_SNAP, 1u, (uint32_t)ZKP_COOP_ST_KNINV, NDev{nullptr, 0});
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = run_prog(d, &v, ZKP_PROG_TW_FROM_SNAP, m, m, 1, nullptr, out + 72 * base, nullptr, nullptr)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// timing hook (diagnostic): one of the synthetic programs (tools/coopgen.py prog_timing; which 0..8), 400 squarings of the
// compressed squaring-run kernel (which 9), the line precomputation of n pairs (which 10) or the one-pair Miller program
// over the line stream it left behind (which 11; call 10 first) - on the caller's stream, timed with the events handed in.
// The kernels' running time does not depend on the data (zeroed buffers serve as inputs).
hipError_t coop_time_prog(CoopState* st, int which, size_t n, hipStream_t s, hipEvent_t e0, hipEvent_t e1, float* ms) {
    CoopDev* d = (CoopDev*)st->d_prog;
    static const int ids[9] = {ZKP_PROG_TIME_T1, ZKP_PROG_TIME_T3, ZKP_PROG_TIME_T3E, ZKP_PROG_TIME_T6, ZKP_PROG_TIME_T12, ZKP_PROG_TIME_LIN,
                               ZKP_PROG_TIME_CYC, ZKP_PROG_TIME_CYCSD, ZKP_PROG_TIME_FILL};
    static const int ids2[3] = {ZKP_PROG_TIME_T6S, ZKP_PROG_TIME_T12S, ZKP_PROG_TIME_T12B};   // which 12..14: one-slot / B-two-slot operand forms
    if (which < 0 || which > 19 || !n || n > 0x7fffffffu || ((which == 10 || which == 11 || which == 15) && n > d->kn.chunk)) return hipErrorInvalidValue;
    hipError_t e = ensure_buf(&d->pipe[0].state, &d->pipe[0].state_bytes, (size_t)ST_SIZE * n * 64);
    if (e != hipSuccess) return e;
    if ((which == 10 || which == 11 || which == 15) && (e = ensure_buf(&d->pipe[0].lines, &d->pipe[0].lines_bytes, (size_t)NLINES * 6 * n * 64)) != hipSuccess) return e;
    CoopPipe v = d->pipe[0];
    v.stream = s;
    bool timed = false;      // which 16 / 17: 57 squarings (one run of the pass) behind ANOTHER kernel (a step program) / behind an idle GPU
    auto once = [&]() -> hipError_t {
        if (which == 9) return run_ksq(s, v.state, (uint32_t)n, (uint32_t)n, 0, 12, 400, 0);   // timing run: no snapshots (a mask needs nsq <= 64)
        if (which >= 16 && which <= 19) {      // 18: behind a ONE-squaring launch of the same grid; 19: behind a step program and that
            if (!timed) {
                timed = true;
                if (which == 17) return hipStreamSynchronize(s);
                if (which == 18) return run_ksq(s, v.state, (uint32_t)n, (uint32_t)n, 0, 12, 1, 0);
                hipError_t e1 = run_prog(d, &v, ZKP_PROG_TIME_T1, (uint32_t)n, (uint32_t)n, 1, nullptr, nullptr, nullptr, nullptr);
                if (e1 != hipSuccess || which == 16) return e1;
                return run_ksq(s, v.state, (uint32_t)n, (uint32_t)n, 0, 12, 1, 0);
            }
            return run_ksq(s, v.state, (uint32_t)n, (uint32_t)n, 0, 12, 57, 0);
        }
        if (which >= 12 && which <= 14) return run_prog(d, &v, ids2[which - 12], (uint32_t)n, (uint32_t)n, 1, nullptr, nullptr, nullptr, nullptr);
        if (which == 10 || which == 15) {                          // 15: the upstream-shaped lines (k_prep_lines<false>)
            const uint64_t* zero = (const uint64_t*)v.state;      // 36 u64 of zeros per pair: the state buffer is far larger
            // (0, 0) is off the twist: 10 times the fused path's twist test and its Jacobian launch, not the CLN steps
            return prep(&v, zero, zero + 12 * n, nullptr, nullptr, 0, (uint32_t)n, 1, 0, 1, which == 10);
        }
        if (which == 11) return run_prog(d, &v, ZKP_PROG_MILLER1_STATE, (uint32_t)n, (uint32_t)n, 1, nullptr, nullptr, nullptr, nullptr);
        return run_prog(d, &v, ids[which], (uint32_t)n, (uint32_t)n, 1, nullptr, nullptr, nullptr, nullptr);
    };
    if (which != 11 && (e = hipMemsetAsync(v.state, 0, (size_t)ST_SIZE * n * 64, s)) != hipSuccess) return e;
    if ((e = once()) != hipSuccess) return e;
    if ((e = hipEventRecord(e0, s)) != hipSuccess) return e;
    if ((e = once()) != hipSuccess) return e;
    if ((e = hipEventRecord(e1, s)) != hipSuccess) return e;
    if ((e = hipEventSynchronize(e1)) != hipSuccess) return e;
    return hipEventElapsedTime(ms, e0, e1);
}

// ZKP_VALID_GENERIC=1 (environment, read once): the compiled kernels alone, the round-3 path - the A/B baseline and the cross-check
static bool valid_generic_only() {
    static const bool v = getenv("ZKP_VALID_GENERIC") && atoi(getenv("ZKP_VALID_GENERIC")) != 0;
    return v;
}
hipError_t coop_g1_valid(const uint64_t* g1, const uint8_t* inf, size_t n, uint8_t* status, hipStream_t s) {
    if (!n) return hipSuccess;
    if (!valid_generic_only()) {
        hipLaunchKernelGGL(k_g1_valid_fast, dim3((unsigned)((n + 63) / 64)), dim3(64), 3 * 4 * 64 * sizeof(int4), s, g1, inf, (uint32_t)n, status);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_g1_valid28, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, g1, inf, (uint32_t)n, status, 1);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_g1_valid28, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, g1, inf, (uint32_t)n, status, 0);
    return hipGetLastError();
}
hipError_t coop_g2_valid(CoopState* st, const uint64_t* g2, const uint8_t* inf, size_t n, uint8_t* status, hipStream_t s) {
    if (!n) return hipSuccess;
    if (!valid_generic_only()) {
        // ZKP_G2_VALID_WAVES=2 (environment, read once): the two-wave kernel (no scratch buffer), the A/B baseline of the three-wave one
        static const bool two_waves = getenv("ZKP_G2_VALID_WAVES") && atoi(getenv("ZKP_G2_VALID_WAVES")) == 2;
        const unsigned blocks = (unsigned)((2 * n + 63) / 64);
        hipError_t e;
        if (two_waves) {
            hipLaunchKernelGGL(k_g2_valid_fast, dim3(blocks), dim3(64), 2 * 4 * 64 * sizeof(int4), s, g2, inf, (uint32_t)n, status);
        } else {
            // at most 2^22 points per launch: the kernel addresses its scratch with 32-bit lane offsets and plane strides (2 lanes x 16 B
            // x 8 planes per point wrap at 2^27 points), and the scratch stays at 1 GiB whatever the batch (launches on one stream
            // run one after the other, so they may share it)
            const size_t CH = plan::VALID_CHUNK;
            CoopDev* d = (CoopDev*)st->d_prog;
            const size_t big = n < CH ? n : CH;
            if ((e = ensure_buf(&d->vscratch, &d->vscratch_bytes, plan::vscratch_bytes(big))) != hipSuccess) return e;
            for (size_t lo = 0; lo < n; lo += CH) {
                const size_t m = n - lo < CH ? n - lo : CH;
                hipLaunchKernelGGL(k_g2_valid_fast3, dim3((unsigned)((2 * m + 63) / 64)), dim3(64), 3 * 4 * 64 * sizeof(int4), s, g2 + 24 * lo,
                                   inf ? inf + lo : nullptr, (uint32_t)m, status + lo, d->vscratch);
            }
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_g2_valid28, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, s, g2, inf, (uint32_t)n, status, 1);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_g2_valid28, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, s, g2, inf, (uint32_t)n, status, 0);
    return hipGetLastError();
}

hipError_t coop_g1_mul(const uint64_t* base, size_t stride, const uint64_t* sc, size_t n, uint64_t* out, uint8_t* out_inf, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_g1_mul28, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, base, stride, sc, (uint32_t)n, out, out_inf);
    return hipGetLastError();
}
hipError_t coop_g2_mul(const uint64_t* base, size_t stride, const uint64_t* sc, size_t n, uint64_t* out, uint8_t* out_inf, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_g2_mul28, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, s, base, stride, sc, (uint32_t)n, out, out_inf);
    return hipGetLastError();
}

hipError_t coop_add(int which, const uint64_t* a, const uint8_t* ia, const uint64_t* b, const uint8_t* ib, size_t n, uint64_t* out, uint8_t* out_inf,
                    hipStream_t s) {
    if (!n) return hipSuccess;
    if (which == 1)
        hipLaunchKernelGGL(k_add28<1>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, a, ia, b, ib, (uint32_t)n, out, out_inf);
    else
        hipLaunchKernelGGL(k_add28<2>, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, s, a, ia, b, ib, (uint32_t)n, out, out_inf);
    return hipGetLastError();
}
hipError_t coop_g1_mul_endo(const uint64_t* base, const uint8_t* inf, const uint64_t* ab, size_t n, uint32_t per, uint64_t* out, uint8_t* out_inf,
                            hipStream_t s) {
    if (!n) return hipSuccess;
    if (!per) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_g1_mul_endo28, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, base, inf, ab, (uint32_t)n, per, out, out_inf);
    return hipGetLastError();
}
hipError_t grp_scale(const uint64_t* base, const uint8_t* inf, const uint64_t* ab, uint32_t n, void* rec, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_grp_scale, dim3((n + 63) / 64), dim3(64), 0, s, base, inf, ab, n, (int4*)rec);
    return hipGetLastError();
}
hipError_t msm_points(const uint64_t* w, uint32_t n_fp, void* rec, hipStream_t s) {
    if (!n_fp) return hipSuccess;
    hipLaunchKernelGGL(k_msm_points, dim3((n_fp + 255) / 256), dim3(256), 0, s, w, n_fp, (int4*)rec);
    return hipGetLastError();
}
hipError_t msm_digits(const uint64_t* sc, const uint8_t* inf, uint32_t terms, uint32_t m, int shared, uint32_t c, uint32_t windows, uint32_t* keys,
                      uint32_t* vals, hipStream_t s) {
    if (!terms) return hipSuccess;
    hipLaunchKernelGGL(k_msm_digits, dim3((terms + 255) / 256), dim3(256), 0, s, sc, inf, terms, m, shared, c, windows, keys, vals);
    return hipGetLastError();
}
hipError_t msm_accum(int which, bool level0, const uint32_t* keys, const uint32_t* vals, const void* src, uint32_t n, uint32_t n_sums, void* sums,
                     uint32_t* okeys, void* oj, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint32_t lanes = (n + msm::RUN - 1) / msm::RUN * (uint32_t)which;
    const dim3 g((lanes + 63) / 64), b(64);
    const int4* r = (const int4*)src;
    if (which == 1 && level0) hipLaunchKernelGGL((k_msm_accum<1, true>), g, b, 0, s, keys, vals, r, n, n_sums, (int4*)sums, okeys, (int4*)oj);
    if (which == 1 && !level0) hipLaunchKernelGGL((k_msm_accum<1, false>), g, b, 0, s, keys, vals, r, n, n_sums, (int4*)sums, okeys, (int4*)oj);
    if (which == 2 && level0) hipLaunchKernelGGL((k_msm_accum<2, true>), g, b, 0, s, keys, vals, r, n, n_sums, (int4*)sums, okeys, (int4*)oj);
    if (which == 2 && !level0) hipLaunchKernelGGL((k_msm_accum<2, false>), g, b, 0, s, keys, vals, r, n, n_sums, (int4*)sums, okeys, (int4*)oj);
    return hipGetLastError();
}
hipError_t msm_reduce(int which, const void* buckets, uint32_t n_sums, uint32_t split, uint32_t chunk, uint32_t* okeys, void* oj, hipStream_t s) {
    const uint32_t lanes = n_sums * split * (uint32_t)which;
    if (!lanes) return hipSuccess;
    if (which == 1)
        hipLaunchKernelGGL(k_msm_reduce<1>, dim3((lanes + 63) / 64), dim3(64), 0, s, (const int4*)buckets, n_sums, split, chunk, okeys, (int4*)oj);
    else
        hipLaunchKernelGGL(k_msm_reduce<2>, dim3((lanes + 63) / 64), dim3(64), 0, s, (const int4*)buckets, n_sums, split, chunk, okeys, (int4*)oj);
    return hipGetLastError();
}
hipError_t msm_final(int which, const void* wsums, uint32_t segs, uint32_t windows, uint32_t c, uint64_t* out, uint8_t* out_inf, hipStream_t s) {
    const uint32_t lanes = segs * (uint32_t)which;
    if (!lanes) return hipSuccess;
    if (which == 1)
        hipLaunchKernelGGL(k_msm_final<1>, dim3((lanes + 63) / 64), dim3(64), 0, s, (const int4*)wsums, segs, windows, c, out, out_inf);
    else
        hipLaunchKernelGGL(k_msm_final<2>, dim3((lanes + 63) / 64), dim3(64), 0, s, (const int4*)wsums, segs, windows, c, out, out_inf);
    return hipGetLastError();
}

hipError_t g1ntt_first(const uint64_t* in, const uint8_t* inf, void* rec, const fk20::First& a, hipStream_t s) {
    if (!a.n_lane) return hipSuccess;
    const dim3 g(fk20::grid(a.n_lane)), b(64);
    if (a.mode == fk20::SRC_REC) hipLaunchKernelGGL(k_g1ntt_first<fk20::SRC_REC>, g, b, 0, s, in, inf, (int4*)rec, a);
    else hipLaunchKernelGGL(k_g1ntt_first<fk20::SRC_WIRE>, g, b, 0, s, in, inf, (int4*)rec, a);
    return hipGetLastError();
}
hipError_t g1ntt_stage(void* rec, const uint64_t* split, const fk20::Stage& a, hipStream_t s) {
    if (!a.n_bfly) return hipSuccess;
    hipLaunchKernelGGL(k_g1ntt_stage, dim3(fk20::grid(a.n_bfly)), dim3(64), 0, s, (int4*)rec, split, a);
    return hipGetLastError();
}
hipError_t g1ntt_out(void* rec, uint64_t* out, uint8_t* out_inf, const fk20::Out& a, const uint64_t* ab, hipStream_t s) {
    if (!a.n_pt) return hipSuccess;
    if (a.scale) {
        hipLaunchKernelGGL(k_g1ntt_scale, dim3(fk20::grid(a.n_pt)), dim3(64), 0, s, (int4*)rec, a, ab[0], ab[1], ab[2], ab[3]);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_g1ntt_out, dim3(fk20::grid(a.n_pt)), dim3(64), 0, s, (const int4*)rec, out, out_inf, a);
    return hipGetLastError();
}
hipError_t fk20_mul(const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* sc, uint32_t n_pt, uint32_t k1, void* rec, hipStream_t s) {
    if (!n_pt) return hipSuccess;
    hipLaunchKernelGGL(k_fk20_mul, dim3(fk20::grid(n_pt)), dim3(64), 0, s, setup, setup_inf, sc, n_pt, k1, (int4*)rec);
    return hipGetLastError();
}
hipError_t cell_mac(const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* sc, void* part, void* rec, const cells::Mac& a, hipStream_t s) {
    if (!a.n_lane) return hipSuccess;
    hipLaunchKernelGGL(k_cell_mac, dim3(fk20::grid(a.n_lane)), dim3(64), cells::mac_lds_bytes(a.s), s, setup, setup_inf, sc, (int4*)part, (int4*)rec, a);
    return hipGetLastError();
}
hipError_t cell_sum(const void* part, void* rec, const cells::Sum& a, hipStream_t s) {
    if (!a.n_lane) return hipSuccess;
    hipLaunchKernelGGL(k_cell_sum, dim3(fk20::grid(a.n_lane)), dim3(64), 0, s, (const int4*)part, (int4*)rec, a);
    return hipGetLastError();
}
hipError_t coop_fp28_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, hipStream_t s) {
    if (!n) return hipSuccess;
    if (op < 0 || op > 5) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fp28_op, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, op, a, b, n, out);
    return hipGetLastError();
}

}  // namespace zkp
