// zkp_bls_minsig.hip -- messages to points of G1 on the GPU (gfx950) and the minimal-signature-size BLS batch verifiers on top of them:
// RFC 9380 BLS12381G1_XMD:SHA-256_SSWU_RO_, signatures in G1, public keys in G2.
//
//   k_g1h_tails    the two tails every message shares (zkp_h2f.hpp's body with I2OSP(128, 2))
//   k_g1h_field    one lane per message: expand_message_xmd to 128 bytes, two wide reductions (zkp_h2f.hpp's body with four blocks)
//   k_g1h_map      one lane per field element u: the straight-line simplified SWU of RFC 9380 F.2 on E1' (Z = 11) with sqrt_ratio for
//                  p = 3 mod 4 - ONE exponentiation by (p - 3) / 4 gives the root, the branch and the division, x stays a fraction -,
//                  the sign from sgn0(u), then the 11-isogeny on the fraction by homogenised Horner steps: a projective point
//                  (X : Y : Z) of E, a pole of the isogeny is the identity (0 : 1 : 0)
//   k_g1h_clear    one lane per point: P = Q0 + Q1 (or a wire point), then [0xd201000000010001] P by a 64-bit double-and-add.  The
//                  group law is the COMPLETE one of Renes, Costello and Batina (algorithms 7 and 9, a = 0): E(Fp) has odd order, so the
//                  same formulas hold for equal points, opposite points and the identity at any step - there is no case to miss
//   k_g1h_affine   the projective sums to affine wire points, one inversion per wavefront of 64 (k_agg_affine's scheme), written with a
//                  stride so that the same-key verifier gets them straight in the rows of its columns
//   k_g1h_init, k_g1h_rows   the verifiers': the flag word and the fixed G2 points; the signatures beside the hashed points
//
// Arithmetic: the 14 x 28-bit carry-free core, one element per lane, every operand in registers (zkp_fp28_ext.hpp).  Limb bounds
// (zkp_fp28.hpp: a two-product form takes operands with La Lb <= 16, a single product La Lb <= 32; a product is L = 1) are given where an
// operand is a sum.
//
// tests/minsig_kernel_host.cpp compiles k_g1h_tails, k_g1h_field, k_g1h_map and k_g1h_clear for the host (ZKP_MINSIG_KERNELS_ONLY) under
// sanitizers and runs them as written; k_g1h_affine exchanges values between lanes and stays on the device.
#ifndef ZKP_MINSIG_KERNELS_ONLY
#include "zkp_bls_minsig.hpp"

#include "zkp_rlc_plan.hpp"
#else
#include "zkp_bls_minsig_plan.hpp"
#endif
#include "zkp_fp28_ext.hpp"
#include "zkp_h2f.hpp"

namespace zkp {
namespace {

using zkp28::Fp28;
using zkp28::NL;
using namespace zkp_f28;

constexpr int TPB_H = 256;   // the hash: a lane per message
constexpr int TPB_M = 64;    // the map, the cofactor, the affine step: a wavefront per workgroup

// A', B', Z, sqrt(-Z), then the isogeny's rows (zkp_constants28.h, generated: tools/gen_constants.py derives them)
__device__ __constant__ const int32_t K_G1H[][NL] = {
#define ZKP_G1H_ROW(name, ...) {__VA_ARGS__},
    ZKP28_G1H_CONST_LIST(ZKP_G1H_ROW)
#undef ZKP_G1H_ROW
};
constexpr int ROW_A = 0, ROW_B = 1, ROW_Z = 2, ROW_C2 = 3, ROW_XNUM = 4, ROW_XDEN = ROW_XNUM + 12, ROW_YNUM = ROW_XDEN + 11, ROW_YDEN = ROW_YNUM + 16;
static_assert(sizeof(K_G1H) == (4 + minsig::ISO_ROWS) * NL * sizeof(int32_t) && ROW_YDEN + 16 == 4 + (int)minsig::ISO_ROWS, "the generated list");

__global__ void k_g1h_tails(const uint8_t* dst, uint32_t dst_len, uint8_t* tail0, uint32_t* tail) {
    if (blockIdx.x || threadIdx.x) return;
    h2f::tails_body(dst, dst_len, (uint32_t)minsig::XMD_BYTES, tail0, tail);
}

// Messages at .. at + n - 1 of n_all; out: n x 2 field elements (u0, u1), 6 words each
__global__ void __launch_bounds__(TPB_H) k_g1h_field(const uint8_t* msgs, const uint64_t* offsets, uint64_t at, uint32_t n, uint64_t n_all, const uint8_t* tail0,
                                                     const uint32_t* tail, uint32_t dst_len, uint64_t* out, int* bad) {
    const uint32_t i = blockIdx.x * TPB_H + threadIdx.x;
    if (i >= n) return;
    h2f::h2f_body<(uint32_t)minsig::XMD_BLOCKS>(msgs, offsets, at, i, n_all, tail0, tail, dst_len, out, bad);
}

// r = take ? a : r per lane, in plain C++ as zkp_bls.hip's f_sel: f_select (zkp_fp28_ext.hpp) is inline asm on a ballot, written for the
// uniform picks out of f_pow_exp's window table, where it keeps the table out of scratch.  The selects here are per-lane and have no
// table behind them, so the compiler is left free to fold them into the neighbouring moves (no spill, no scratch: the code objects).
__device__ __forceinline__ void f_sel(Fp28& r, const Fp28& a, bool take) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = take ? a.l[i] : r.l[i];
}
__device__ __forceinline__ void f_zero(Fp28& r) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = 0;
}
// a projective point in a workspace: limb k of coordinate v of slot s at ws[(14 v + k) stride + s] (a lane's accesses are coalesced
// across the wavefront)
__device__ __forceinline__ void f_st(int32_t* ws, size_t stride, size_t slot, int at, const Fp28& a) {
#pragma unroll
    for (int i = 0; i < NL; i++) ws[(size_t)(at + i) * stride + slot] = a.l[i];
}
__device__ __forceinline__ void f_ld(Fp28& a, const int32_t* ws, size_t stride, size_t slot, int at) {
#pragma unroll
    for (int i = 0; i < NL; i++) a.l[i] = ws[(size_t)(at + i) * stride + slot];
}

// ------------------------------------------------------------------------------------------- the map
// u: m field elements (6 words each, canonical); slot t of the workspace receives iso(sswu(u_t))
__global__ void __launch_bounds__(TPB_M) k_g1h_map(const uint64_t* u, uint32_t m, int32_t* ws, size_t stride) {
    const uint32_t t = blockIdx.x * TPB_M + threadIdx.x;
    if (t >= m) return;
    const uint64_t* uw = u + 6 * (size_t)t;
    const uint32_t sgn_u = (uint32_t)(uw[0] & 1);
    Fp28 uu, ka, kb, kz, one, tv1, tv2, tv3, tv4, tv5, tv6, xn, y;
    zkp28::fp28_from_wire(uu, uw);
    f_const(ka, K_G1H[ROW_A]);
    f_const(kb, K_G1H[ROW_B]);
    f_const(kz, K_G1H[ROW_Z]);
    f_const(one, zkp28::K28_ONE);
    // RFC 9380 F.2, the names of its steps
    f_sqr(tv1, uu);
    f_mul(tv1, kz, tv1);                                           // Z u^2
    f_sqr(tv2, tv1);
    f_add(tv2, tv2, tv1);                                          // Z^2 u^4 + Z u^2: L2
    f_add(tv3, tv2, one);                                          // L3
    f_mul(tv3, kb, tv3);                                           // B (tv2 + 1): x1's numerator
    const bool exceptional = f_is_zero(tv2);                       // u = 0 and u = +-sqrt(-1 / Z)
    f_neg(tv4, tv2);
    f_sel(tv4, kz, exceptional);
    f_mul(tv4, ka, tv4);                                           // A (-tv2), or A Z: the denominator of x, never zero
    f_sqr(tv2, tv3);
    f_sqr(tv6, tv4);
    f_mul(tv5, ka, tv6);
    f_add(tv2, tv2, tv5);                                          // L2
    f_mul(tv2, tv2, tv3);
    f_mul(tv6, tv6, tv4);                                          // tv4^3
    f_mul(tv5, kb, tv6);
    f_add(tv2, tv2, tv5);                                          // g(x1)'s numerator over tv6: L2
    f_mul(xn, tv1, tv3);                                           // x2's numerator
    // sqrt_ratio(tv2, tv6) for p = 3 mod 4 (F.2.1.2): y1 = (u v^3)^((p-3)/4) u v
    Fp28 v2, uv, e, y1, y2;
    f_sqr(v2, tv6);
    f_mul(uv, tv2, tv6);
    f_mul(v2, v2, uv);
    f_pow_exp(e, v2);
    f_mul(y1, e, uv);
    f_const(e, K_G1H[ROW_C2]);
    f_mul(y2, y1, e);                                              // the root of Z g(x1) when g(x1) is no square
    f_sqr(e, y1);
    f_mul(e, e, tv6);
    const bool square = f_eq(e, tv2);
    f_mul(y, tv1, uu);
    f_mul(y, y, y2);                                               // Z u^3 sqrt(Z g(x1)): the root of g(x2)
    f_sel(xn, tv3, square);
    f_sel(y, y1, square);
    uint64_t yw[6];
    zkp28::fp28_to_wire(yw, y);
    Fp28 ny;
    f_neg(ny, y);
    f_sel(y, ny, (uint32_t)(yw[0] & 1) != sgn_u);
    // the 11-isogeny at x = xn / xd, xd = tv4: Horner from the top coefficient, step j adds (the next coefficient) xd^j, so that after its
    // last step a polynomial of degree n holds xd^n times its value.  x_num: 11 steps, x_den: 10, y_num and y_den: 15.
    Fp28 pd = tv4, axn, axd, ayn, ayd, k;
    f_const(axn, K_G1H[ROW_XNUM + 11]);
    f_const(axd, K_G1H[ROW_XDEN + 10]);
    f_const(ayn, K_G1H[ROW_YNUM + 15]);
    f_const(ayd, K_G1H[ROW_YDEN + 15]);
#pragma unroll 1
    for (int j = 1; j <= 15; j++) {
        if (j > 1) f_mul(pd, pd, tv4);
        if (j <= 11) {
            f_const(k, K_G1H[ROW_XNUM + 11 - j]);
            f_mul2(axn, axn, xn, k, pd);
        }
        if (j <= 10) {
            f_const(k, K_G1H[ROW_XDEN + 10 - j]);
            f_mul2(axd, axd, xn, k, pd);
        }
        f_const(k, K_G1H[ROW_YNUM + 15 - j]);
        f_mul2(ayn, ayn, xn, k, pd);
        f_const(k, K_G1H[ROW_YDEN + 15 - j]);
        f_mul2(ayd, ayd, xn, k, pd);
    }
    // x = axn / (xd axd), y = y ayn / ayd: the point (axn ayd : y ayn xd axd : xd axd ayd)
    Fp28 qx, qy, qz;
    f_mul(axd, axd, tv4);
    f_mul(qx, axn, ayd);
    f_mul(qz, axd, ayd);
    f_mul(qy, y, ayn);
    f_mul(qy, qy, axd);
    const bool pole = f_is_zero(qz);
    f_zero(k);
    f_sel(qx, k, pole);
    f_sel(qz, k, pole);
    f_sel(qy, one, pole);
    f_st(ws, stride, t, 0, qx);
    f_st(ws, stride, t, NL, qy);
    f_st(ws, stride, t, 2 * NL, qz);
}

// ------------------------------------------------------------------------------------------- the complete group law on E: y^2 = x^3 + 4
struct Pt { Fp28 x, y, z; };
// Renes-Costello-Batina, algorithm 7 (a = 0, b3 = 12).  p of L <= 2, q of L <= 2: every product below has La Lb <= 16; r of L <= 2
__device__ __forceinline__ void pt_add(Pt& r, const Pt& p, const Pt& q, const Fp28& b3) {
    Fp28 t0, t1, t2, t3, t4, x3, y3, z3;
    f_mul(t0, p.x, q.x);
    f_mul(t1, p.y, q.y);
    f_mul(t2, p.z, q.z);
    f_add(t3, p.x, p.y);
    f_add(t4, q.x, q.y);
    f_mul(t3, t3, t4);
    f_add(t4, t0, t1);
    f_sub(t3, t3, t4);                                             // L3
    f_add(t4, p.y, p.z);
    f_add(x3, q.y, q.z);
    f_mul(t4, t4, x3);
    f_add(x3, t1, t2);
    f_sub(t4, t4, x3);                                             // L3
    f_add(x3, p.x, p.z);
    f_add(y3, q.x, q.z);
    f_mul(x3, x3, y3);
    f_add(y3, t0, t2);
    f_sub(y3, x3, y3);                                             // L3
    f_add(x3, t0, t0);
    f_add(t0, x3, t0);                                             // L3
    f_mul(t2, b3, t2);
    f_add(z3, t1, t2);                                             // L2
    f_sub(t1, t1, t2);                                             // L2
    f_mul(y3, b3, y3);
    f_mul(x3, t4, y3);
    f_mul(t2, t3, t1);
    f_sub(x3, t2, x3);
    f_mul(y3, y3, t0);
    f_mul(t1, t1, z3);
    f_add(y3, t1, y3);
    f_mul(t0, t0, t3);
    f_mul(z3, z3, t4);
    f_add(z3, z3, t0);
    r.x = x3;
    r.y = y3;
    r.z = z3;
}
// algorithm 9 (a = 0).  p of L <= 2; r.x, r.y of L 2, r.z of L 1
__device__ __forceinline__ void pt_dbl(Pt& r, const Pt& p, const Fp28& b3) {
    Fp28 t0, t1, t2, x3, y3, z3;
    f_sqr(t0, p.y);
    f_add(z3, t0, t0);
    f_add(z3, z3, z3);
    f_add(z3, z3, z3);                                             // 8 y^2: L8, met by L1 operands only
    f_mul(t1, p.y, p.z);
    f_sqr(t2, p.z);
    f_mul(t2, b3, t2);
    f_mul(x3, t2, z3);
    f_add(y3, t0, t2);
    f_mul(z3, t1, z3);
    f_add(t1, t2, t2);
    f_add(t2, t1, t2);                                             // L3
    f_sub(t0, t0, t2);                                             // L4
    f_mul(y3, t0, y3);
    f_add(y3, x3, y3);
    f_mul(t1, p.x, p.y);
    f_mul(x3, t0, t1);
    f_add(x3, x3, x3);
    r.x = x3;
    r.y = y3;
    r.z = z3;
}

// ------------------------------------------------------------------------------------------- the sum and the cofactor
// WIRE: point i is the wire point pts[i] (any point of the curve; inf may be null); otherwise it is the sum of slots 2 i and 2 i + 1 of
// `in`.  Slot i of `out` receives [1 - x] of it, projective.
template <bool WIRE>
__global__ void __launch_bounds__(TPB_M) k_g1h_clear(const uint64_t* pts, const uint8_t* inf, const int32_t* in, size_t in_stride, uint32_t n, int32_t* out,
                                                     size_t out_stride) {
    const uint32_t i = blockIdx.x * TPB_M + threadIdx.x;
    if (i >= n) return;
    Fp28 b3, one, kb;
    f_const(one, zkp28::K28_ONE);
    f_const(kb, zkp28::K28_B);
    f_add(b3, kb, kb);
    f_add(b3, b3, kb);                                             // 3 b = 12: L3, met by L <= 3 operands only
    Pt p;
    if (WIRE) {
        zkp28::fp28_from_wire(p.x, pts + 12 * (size_t)i);
        zkp28::fp28_from_wire(p.y, pts + 12 * (size_t)i + 6);
        p.z = one;
        const bool at_inf = inf && inf[i];
        Fp28 zero;
        f_zero(zero);
        f_sel(p.x, zero, at_inf);
        f_sel(p.y, one, at_inf);
        f_sel(p.z, zero, at_inf);
    } else {
        Pt q0, q1;
        f_ld(q0.x, in, in_stride, 2 * (size_t)i, 0);
        f_ld(q0.y, in, in_stride, 2 * (size_t)i, NL);
        f_ld(q0.z, in, in_stride, 2 * (size_t)i, 2 * NL);
        f_ld(q1.x, in, in_stride, 2 * (size_t)i + 1, 0);
        f_ld(q1.y, in, in_stride, 2 * (size_t)i + 1, NL);
        f_ld(q1.z, in, in_stride, 2 * (size_t)i + 1, 2 * NL);
        pt_add(p, q0, q1, b3);
    }
    // MSB first from the top bit, which is set: a doubling per bit, an addition per set bit (six of them)
    Pt r = p;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        pt_dbl(r, r, b3);
        if ((minsig::H_EFF >> b) & 1) pt_add(r, r, p, b3);
    }
    f_st(out, out_stride, i, 0, r.x);
    f_st(out, out_stride, i, NL, r.y);
    f_st(out, out_stride, i, 2 * NL, r.z);
}

#ifndef ZKP_MINSIG_KERNELS_ONLY
// ------------------------------------------------------------------------------------------- projective sums -> affine wire points
// a value per lane in LDS, plane pl (limb quad q of lane l at [(pl * 4 + q) * 64 + l]: a lane's four stores and loads are conflict-free)
__device__ __forceinline__ void sh_st(int4* sh, int pl, int lane, const Fp28& x) {
    sh[(pl * 4 + 0) * 64 + lane] = make_int4(x.l[0], x.l[1], x.l[2], x.l[3]);
    sh[(pl * 4 + 1) * 64 + lane] = make_int4(x.l[4], x.l[5], x.l[6], x.l[7]);
    sh[(pl * 4 + 2) * 64 + lane] = make_int4(x.l[8], x.l[9], x.l[10], x.l[11]);
    sh[(pl * 4 + 3) * 64 + lane] = make_int4(x.l[12], x.l[13], 0, 0);
}
__device__ __forceinline__ void sh_ld(Fp28& x, const int4* sh, int pl, int lane) {
    const int4 v0 = sh[(pl * 4 + 0) * 64 + lane], v1 = sh[(pl * 4 + 1) * 64 + lane], v2 = sh[(pl * 4 + 2) * 64 + lane], v3 = sh[(pl * 4 + 3) * 64 + lane];
    x.l[0] = v0.x; x.l[1] = v0.y; x.l[2] = v0.z; x.l[3] = v0.w; x.l[4] = v1.x; x.l[5] = v1.y; x.l[6] = v1.z; x.l[7] = v1.w;
    x.l[8] = v2.x; x.l[9] = v2.y; x.l[10] = v2.z; x.l[11] = v2.w; x.l[12] = v3.x; x.l[13] = v3.y;
}

// One lane per point, a wavefront per workgroup: 1 / Z_l for the 64 points of a wavefront from ONE inversion, by inclusive prefix and
// suffix products through LDS (k_agg_affine's scheme, zkp_bls_agg.hip; that kernel reads Jacobian records, this one projective planes).
// The identity (Z = 0) and the lanes past n enter the chain as 1; the identity comes out as (0, 1) with out_inf = 1.  Point j goes to
// row j * ostride of out / out_inf.
__global__ void __launch_bounds__(TPB_M) k_g1h_affine(const int32_t* in, size_t stride, uint32_t n, uint64_t* out, uint8_t* out_inf, uint32_t ostride) {
    __shared__ int4 sh[2 * 4 * 64];
    const int lane = threadIdx.x;
    const uint32_t j = blockIdx.x * TPB_M + lane;
    const bool live = j < n;
    const uint32_t jj = live ? j : n - 1;
    Fp28 one, z;
    f_const(one, zkp28::K28_ONE);
    f_ld(z, in, stride, jj, 2 * NL);
    const bool dead = !live || f_is_zero(z);
    f_sel(z, one, dead);
    Fp28 pre = z, suf = z;
#pragma unroll 1
    for (int d = 1; d < 64; d *= 2) {
        sh_st(sh, 0, lane, pre);
        sh_st(sh, 1, lane, suf);
        __syncthreads();
        const bool dn = lane >= d, up = lane + d < 64;
        Fp28 a, b;
        sh_ld(a, sh, 0, dn ? lane - d : lane);
        sh_ld(b, sh, 1, up ? lane + d : lane);
        __syncthreads();
        f_mul(a, pre, a);
        f_mul(b, suf, b);
        f_sel(pre, a, dn);
        f_sel(suf, b, up);
    }
    sh_st(sh, 0, lane, pre);
    sh_st(sh, 1, lane, suf);
    __syncthreads();
    Fp28 total, before = one, after = one, zi, t, ax, ay;
    sh_ld(total, sh, 0, 63);
    sh_ld(t, sh, 0, lane ? lane - 1 : 0);
    f_sel(before, t, lane > 0);
    sh_ld(t, sh, 1, lane < 63 ? lane + 1 : 63);
    f_sel(after, t, lane < 63);
    f_mul(before, before, after);
    {   // 1 / total = (total^((p-3)/4))^4 total
        Fp28 e;
        f_pow_exp(e, total);
        f_sqr(e, e);
        f_sqr(e, e);
        f_mul(t, e, total);
    }
    f_mul(zi, before, t);
    f_ld(t, in, stride, jj, 0);
    f_mul(ax, t, zi);
    f_ld(t, in, stride, jj, NL);
    f_mul(ay, t, zi);
    if (!live) return;
    uint64_t wx[6], wy[6];
    zkp28::fp28_to_wire(wx, ax);
    zkp28::fp28_to_wire(wy, ay);
    const size_t row = (size_t)j * ostride;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        out[12 * row + k] = dead ? 0 : wx[k];
        out[12 * row + 6 + k] = dead ? (k == 0 ? 1 : 0) : wy[k];
    }
    out_inf[row] = dead ? 1 : 0;
}

// ------------------------------------------------------------------------------------------- the verifiers' small kernels
// flag[0] = 0 (nothing refuses the batch yet), or 1 when the same-key verifier's key is the identity as the wire writes it, (0, 1);
// fixed: -g2 as a wire point, behind the key when there is one
__global__ void k_g1h_init(int* flag, const uint64_t* pk, uint64_t* fixed, uint8_t* fixed_inf) {
    if (blockIdx.x || threadIdx.x) return;
    int refuse = 0;
    uint64_t* neg = fixed;
    if (pk) {
        uint64_t rest = 0;
        for (int k = 0; k < 24; k++) {
            fixed[k] = pk[k];
            if (k != 12) rest |= pk[k];
        }
        refuse = rest == 0 && pk[12] == 1;
        neg = fixed + 24;
        fixed_inf[1] = 0;
    }
    flag[0] = refuse;
    fixed_inf[0] = 0;
    Fp28 v;
    f_const(v, zkp28::K28_G2_X0);
    zkp28::fp28_to_wire(neg, v);
    f_const(v, zkp28::K28_G2_X1);
    zkp28::fp28_to_wire(neg + 6, v);
    f_const(v, zkp28::K28_G2_Y0);
    f_neg(v, v);
    zkp28::fp28_to_wire(neg + 12, v);
    f_const(v, zkp28::K28_G2_Y1);
    f_neg(v, v);
    zkp28::fp28_to_wire(neg + 18, v);
}
// the same-key verifier's rows: signature i beside the hashed point, row 2 i + 1 (inf_sig may be null)
__global__ void __launch_bounds__(TPB_H) k_g1h_rows(const uint64_t* sig, const uint8_t* inf_sig, size_t n, uint64_t* rows, uint8_t* rows_inf) {
    const size_t t = (size_t)blockIdx.x * TPB_H + threadIdx.x;
    if (t >= 12 * n) return;
    const size_t i = t / 12, k = t % 12;
    rows[12 * (2 * i + 1) + k] = sig[t];
    if (k == 0) rows_inf[2 * i + 1] = inf_sig ? inf_sig[i] : 0;
}
// any non-zero status byte refuses the batch (every writer stores the same 1: a plain store, as k_bls_fold's)
__global__ void __launch_bounds__(TPB_H) k_g1h_fold(const uint8_t* st, size_t n, int* flag) {
    const size_t i = (size_t)blockIdx.x * TPB_H + threadIdx.x;
    if (i < n && st[i]) flag[0] = 1;
}
__global__ void k_g1h_finish(const int* flag, int* all_ok) {
    if (flag[0]) *all_ok = 0;
}

inline unsigned blocks_of(size_t n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

#define G1H_CHK(c, what, call)                                        \
    do {                                                              \
        if (int rc__ = ctxop::fail((c), (what), (call))) return rc__; \
    } while (0)

int tails(zkp_ctx* c, const minsig::Layout& L, char* w, const void* dst, size_t dst_len, hipStream_t s) {
    hipLaunchKernelGGL(k_g1h_tails, dim3(1), dim3(1), 0, s, (const uint8_t*)dst, (uint32_t)dst_len, (uint8_t*)(w + L.tail0), (uint32_t*)(w + L.tail));
    return ctxop::fail(c, "k_g1h_tails", hipGetLastError());
}
int field_slice(zkp_ctx* c, const minsig::Layout& L, char* w, const void* msgs, const void* offsets, size_t at, size_t cnt, size_t n_all, size_t dst_len,
                uint64_t* out_u, hipStream_t s) {
    hipLaunchKernelGGL(k_g1h_field, dim3(blocks_of(cnt, TPB_H)), dim3(TPB_H), 0, s, (const uint8_t*)msgs, (const uint64_t*)offsets, (uint64_t)at, (uint32_t)cnt,
                       (uint64_t)n_all, (const uint8_t*)(w + L.tail0), (const uint32_t*)(w + L.tail), (uint32_t)dst_len, out_u, ctxop::bls_bad_word(c));
    return ctxop::fail(c, "k_g1h_field", hipGetLastError());
}
// the slice's cleared sums (cnt <= L.slice of them) to wire points, point j at row j * ostride
int affine_slice(zkp_ctx* c, const minsig::Layout& L, char* w, size_t cnt, uint64_t* out, uint8_t* out_inf, size_t ostride, hipStream_t s) {
    hipLaunchKernelGGL(k_g1h_affine, dim3(blocks_of(cnt, TPB_M)), dim3(TPB_M), 0, s, (const int32_t*)(w + L.sums), L.slice, (uint32_t)cnt, out, out_inf,
                       (uint32_t)ostride);
    return ctxop::fail(c, "k_g1h_affine", hipGetLastError());
}
// cnt <= L.slice points: u (device, cnt x 2 Fp) through the map, the sum, the cofactor and the affine step
int map_slice(zkp_ctx* c, const minsig::Layout& L, char* w, const uint64_t* u, size_t cnt, uint64_t* out, uint8_t* out_inf, size_t ostride, hipStream_t s) {
    int32_t *pts = (int32_t*)(w + L.pts), *sums = (int32_t*)(w + L.sums);
    hipLaunchKernelGGL(k_g1h_map, dim3(blocks_of(2 * cnt, TPB_M)), dim3(TPB_M), 0, s, u, (uint32_t)(2 * cnt), pts, 2 * L.slice);
    G1H_CHK(c, "k_g1h_map", hipGetLastError());
    hipLaunchKernelGGL(k_g1h_clear<false>, dim3(blocks_of(cnt, TPB_M)), dim3(TPB_M), 0, s, (const uint64_t*)nullptr, (const uint8_t*)nullptr, (const int32_t*)pts,
                       2 * L.slice, (uint32_t)cnt, sums, L.slice);
    G1H_CHK(c, "k_g1h_clear", hipGetLastError());
    return affine_slice(c, L, w, cnt, out, out_inf, ostride, s);
}
// the composition, slice by slice: the u values of a slice stay in the workspace
int hash_into(zkp_ctx* c, const minsig::Layout& L, char* w, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, uint64_t* out,
              uint8_t* out_inf, size_t ostride, hipStream_t s) {
    int rc = tails(c, L, w, dst, dst_len, s);
    uint64_t* u = (uint64_t*)(w + L.u);
    for (size_t at = 0; at < n && !rc; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        if ((rc = field_slice(c, L, w, msgs, offsets, at, cnt, n, dst_len, u, s))) break;
        rc = map_slice(c, L, w, u, cnt, out + 12 * at * ostride, out_inf + at * ostride, ostride, s);
    }
    return rc;
}
int fold(zkp_ctx* c, const uint8_t* st, size_t n, int* flag, hipStream_t s) {
    hipLaunchKernelGGL(k_g1h_fold, dim3(blocks_of(n, TPB_H)), dim3(TPB_H), 0, s, st, n, flag);
    return ctxop::fail(c, "k_g1h_fold", hipGetLastError());
}

}  // namespace

int g1h_field_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out_u, hipStream_t s) {
    if (!n) return 0;
    const minsig::Layout L = minsig::layout(n, minsig::HASH);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_minsig(c, L.total, &ws)) || (rc = tails(c, L, (char*)ws, dst, dst_len, s))) return rc;
    for (size_t at = 0; at < n && !rc; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        rc = field_slice(c, L, (char*)ws, msgs, offsets, at, cnt, n, dst_len, (uint64_t*)out_u + 12 * at, s);
    }
    return rc;
}

int g1h_map_dev(zkp_ctx* c, const void* u, size_t n, void* out, void* out_inf, hipStream_t s) {
    if (!n) return 0;
    const minsig::Layout L = minsig::layout(n, minsig::HASH);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_minsig(c, L.total, &ws))) return rc;
    for (size_t at = 0; at < n && !rc; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        rc = map_slice(c, L, (char*)ws, (const uint64_t*)u + 12 * at, cnt, (uint64_t*)out + 12 * at, (uint8_t*)out_inf + at, 1, s);
    }
    return rc;
}

int g1h_clear_dev(zkp_ctx* c, const void* pts, const void* inf, size_t n, void* out, void* out_inf, hipStream_t s) {
    if (!n) return 0;
    const minsig::Layout L = minsig::layout(n, minsig::HASH);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_minsig(c, L.total, &ws))) return rc;
    char* w = (char*)ws;
    for (size_t at = 0; at < n && !rc; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        hipLaunchKernelGGL(k_g1h_clear<true>, dim3(blocks_of(cnt, TPB_M)), dim3(TPB_M), 0, s, (const uint64_t*)pts + 12 * at,
                           inf ? (const uint8_t*)inf + at : (const uint8_t*)nullptr, (const int32_t*)nullptr, (size_t)0, (uint32_t)cnt, (int32_t*)(w + L.sums), L.slice);
        G1H_CHK(c, "k_g1h_clear", hipGetLastError());
        rc = affine_slice(c, L, w, cnt, (uint64_t*)out + 12 * at, (uint8_t*)out_inf + at, 1, s);
    }
    return rc;
}

int g1h_hash_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out, void* out_inf, hipStream_t s) {
    if (!n) return 0;
    const minsig::Layout L = minsig::layout(n, minsig::HASH);
    void* ws = nullptr;
    if (int rc = ctxop::grow_minsig(c, L.total, &ws)) return rc;
    return hash_into(c, L, (char*)ws, msgs, offsets, n, dst, dst_len, (uint64_t*)out, (uint8_t*)out_inf, 1, s);
}

int minsig_verify_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig,
                      const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s) {
    zkp_rlc_batch b = {};
    if (!n) return rlc_check_dev(c, &b, nullptr, ZKP_RLC_POINTS_CHECKED, all_ok, s);       // the empty batch holds
    const minsig::Layout L = minsig::layout(n, minsig::VERIFY);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_minsig(c, L.total, &ws))) return rc;
    char* w = (char*)ws;
    int* flag = (int*)(w + L.flag);
    uint64_t* hp = (uint64_t*)(w + L.hp);
    uint8_t *hinf = (uint8_t*)(w + L.hinf), *st = (uint8_t*)(w + L.st);
    hipLaunchKernelGGL(k_g1h_init, dim3(1), dim3(1), 0, s, flag, (const uint64_t*)nullptr, (uint64_t*)(w + L.fixed_g2), (uint8_t*)(w + L.fixed_inf2));
    G1H_CHK(c, "k_g1h_init", hipGetLastError());
    if (!(flags & 1)) {                                            // ZKP_BLS_POINTS_CHECKED
        if ((rc = ctxop::valid(c, 2, pk, inf_pk, n, st, s)) || (rc = ctxop::valid(c, 1, sig, inf_sig, n, st + n, s)) || (rc = fold(c, st, 2 * n, flag, s))) return rc;
    }
    if (inf_pk && (rc = fold(c, (const uint8_t*)inf_pk, n, flag, s))) return rc;          // KeyValidate: the identity is no public key
    if ((rc = hash_into(c, L, w, msgs, offsets, n, dst, dst_len, hp, hinf, 1, s))) return rc;
    // prod_i e([r_i] H(m_i), pk_i) e(sum_i [r_i] sig_i, -g2): one free pair per check and one column with the fixed -g2
    b.n_checks = n;
    b.k = 1;
    b.g1 = hp;
    b.g2 = pk;
    b.inf1 = hinf;
    b.inf2 = inf_pk;
    b.s2 = 1;
    b.col_g1 = sig;
    b.col_inf1 = inf_sig;
    b.fixed_g2 = w + L.fixed_g2;
    b.fixed_inf2 = w + L.fixed_inf2;
    if ((rc = rlc_check_dev(c, &b, (const uint64_t*)rand, ZKP_RLC_POINTS_CHECKED, all_ok, s))) return rc;
    hipLaunchKernelGGL(k_g1h_finish, dim3(1), dim3(1), 0, s, (const int*)flag, all_ok);
    return ctxop::fail(c, "k_g1h_finish", hipGetLastError());
}

int minsig_verify_samekey_dev(zkp_ctx* c, const void* pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig,
                              const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s) {
    zkp_rlc_batch b = {};
    if (!n) return rlc_check_dev(c, &b, nullptr, ZKP_RLC_POINTS_CHECKED, all_ok, s);       // the empty batch holds
    const minsig::Layout L = minsig::layout(n, minsig::SAMEKEY);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_minsig(c, L.total, &ws))) return rc;
    char* w = (char*)ws;
    int* flag = (int*)(w + L.flag);
    uint64_t* rows = (uint64_t*)(w + L.hp);
    uint8_t *rows_inf = (uint8_t*)(w + L.hinf), *st = (uint8_t*)(w + L.st);
    hipLaunchKernelGGL(k_g1h_init, dim3(1), dim3(1), 0, s, flag, (const uint64_t*)pk, (uint64_t*)(w + L.fixed_g2), (uint8_t*)(w + L.fixed_inf2));
    G1H_CHK(c, "k_g1h_init", hipGetLastError());
    if (!(flags & 1)) {                                            // ZKP_BLS_POINTS_CHECKED
        if ((rc = ctxop::valid(c, 1, sig, inf_sig, n, st, s)) || (rc = ctxop::valid(c, 2, pk, nullptr, 1, st + n, s)) || (rc = fold(c, st, n + 1, flag, s))) return rc;
    }
    // the hashed points go straight into the even rows of the n x 2 column layout, the signatures into the odd ones
    if ((rc = hash_into(c, L, w, msgs, offsets, n, dst, dst_len, rows, rows_inf, 2, s))) return rc;
    hipLaunchKernelGGL(k_g1h_rows, dim3(blocks_of(12 * n, TPB_H)), dim3(TPB_H), 0, s, (const uint64_t*)sig, (const uint8_t*)inf_sig, n, rows, rows_inf);
    G1H_CHK(c, "k_g1h_rows", hipGetLastError());
    // e(sum_i [r_i] H(m_i), pk) e(sum_i [r_i] sig_i, -g2): no free pair, two columns
    b.n_checks = n;
    b.k = 0;
    b.s2 = 2;
    b.col_g1 = rows;
    b.col_inf1 = rows_inf;
    b.fixed_g2 = w + L.fixed_g2;
    b.fixed_inf2 = w + L.fixed_inf2;
    if ((rc = rlc_check_dev(c, &b, (const uint64_t*)rand, ZKP_RLC_POINTS_CHECKED, all_ok, s))) return rc;
    hipLaunchKernelGGL(k_g1h_finish, dim3(1), dim3(1), 0, s, (const int*)flag, all_ok);
    return ctxop::fail(c, "k_g1h_finish", hipGetLastError());
}

#else
}  // namespace
#endif

}  // namespace zkp
