// zkp_bls.hip -- messages to points of G2 on the GPU (gfx950) and the BLS batch verifier on top of them: RFC 9380
// BLS12381G2_XMD:SHA-256_SSWU_RO_, public keys in G1, signatures in G2.
//
//   k_h2c_tails   the two tails every message shares, from the DST in device memory: what b_0 absorbs after the message, and the padded
//                 remainder of every b_i block chain as big-endian words
//   k_h2f         one lane per message: expand_message_xmd to 256 bytes (SHA-256, the schedule in 16 rolling registers, no LDS), each
//                 64-byte slice reduced mod p straight from the registers: hi 2^256 + lo as ONE two-product Montgomery reduction
//   k_h2c_wide    the reduction alone, on 64 big-endian bytes per element (zkp_fp_from_wide_be_batch)
//   k_h2c_map     one lane per field element u: simplified SWU on E' (y^2 = x^3 + 240 i x + 1012 (1 + i), Z = -(2 + i)), the sign of y,
//                 the 3-isogeny to E2 - a projective point (x_num d : y y_num : d^3), d = x' + 6 - 6 i, so a pole is the identity
//   k_h2c_clear   (zkp_bls_clear.hip, two lanes per point) P = Q0 + Q1, then
//                 [x^2 - x - 1] P + [x - 1] psi(P) + psi^2(2 P) by two 64-bit ladders, one inversion to the affine wire point
//
// Arithmetic: the 14 x 28-bit carry-free core, one element per lane, every operand in registers (zkp_fp28_ext.hpp) - the family of
// k_g2_decompress, whose two exponentiations this file reuses.  Per u: the inversion of Z^2 u^4 + Z u^2 (one exponentiation), the norm's
// root of g(x1) (one; it also decides the branch: g(x1) is a square iff its norm is, and for a non-square the root of norm(Z^3 g(x1)) is
// that root times a constant) and the root's second exponentiation: 3 x 461 products, against about 2500 for a single-exponentiation
// sqrt_ratio over Fp2.
//
// Limb bounds (zkp_fp28.hpp: a two-product form takes operands with La Lb <= 16, a single product La Lb <= 32, in units of 2^27; a
// product is L = 1): the comments below give the bound of the operands that are sums.
//
// tests/bls_kernel_host.cpp compiles the hash kernels of this file (k_h2c_tails, k_h2f, k_h2c_wide: SHA-256, the expander, the wide reduction)
// for the host (ZKP_BLS_KERNELS_ONLY) under sanitizers and runs them as written on exactly allocated buffers.
#ifndef ZKP_BLS_KERNELS_ONLY
#include "zkp_bls.hpp"

#include "zkp_coop.hpp"
#include "zkp_fp28_ext.hpp"
#include "zkp_rlc_plan.hpp"
#else
#include "zkp_bls_plan.hpp"
#include "zkp_fp28.hpp"
#endif
#include "zkp_h2f.hpp"

namespace zkp {
namespace {

using zkp28::Fp28;
using zkp28::NL;
#ifndef ZKP_BLS_KERNELS_ONLY
using namespace zkp_f28;
#endif

constexpr int TPB_H = 256;   // the hash: a lane per message
constexpr int TPB_M = 64;    // the map: a wavefront per workgroup, the register file to itself

// SHA-256, the expander and the wide reduction: zkp_h2f.hpp, shared with zkp_bls_minsig.hip
using h2f::reduce_wide;

__global__ void k_h2c_tails(const uint8_t* dst, uint32_t dst_len, uint8_t* tail0, uint32_t* tail) {
    if (blockIdx.x || threadIdx.x) return;
    h2f::tails_body(dst, dst_len, (uint32_t)bls::XMD_BYTES, tail0, tail);
}

// Messages at .. at + n - 1 of n_all; out: n x 4 field elements (u0.c0, u0.c1, u1.c0, u1.c1), 6 words each (the body: zkp_h2f.hpp)
__global__ void __launch_bounds__(TPB_H) k_h2f(const uint8_t* msgs, const uint64_t* offsets, uint64_t at, uint32_t n, uint64_t n_all, const uint8_t* tail0,
                                               const uint32_t* tail, uint32_t dst_len, uint64_t* out, int* bad) {
    const uint32_t i = blockIdx.x * TPB_H + threadIdx.x;
    if (i >= n) return;
    h2f::h2f_body<(uint32_t)bls::XMD_BLOCKS>(msgs, offsets, at, i, n_all, tail0, tail, dst_len, out, bad);
}

__global__ void __launch_bounds__(TPB_H) k_h2c_wide(const uint8_t* bytes, size_t n, uint64_t* out) {
    const size_t i = (size_t)blockIdx.x * TPB_H + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = bytes + 64 * i;
    uint32_t be[16];
#pragma unroll
    for (int k = 0; k < 16; k++) be[k] = ((uint32_t)p[4 * k] << 24) | ((uint32_t)p[4 * k + 1] << 16) | ((uint32_t)p[4 * k + 2] << 8) | p[4 * k + 3];
    uint64_t o[6];
    reduce_wide(o, be, be + 8);
#pragma unroll
    for (int k = 0; k < 6; k++) out[6 * i + k] = o[k];
}

#ifndef ZKP_BLS_KERNELS_ONLY
// ------------------------------------------------------------------------------------------- Fp2 on the 28-bit core
__device__ __forceinline__ void f2_add(F2& r, const F2& a, const F2& b) { f_add(r.c0, a.c0, b.c0); f_add(r.c1, a.c1, b.c1); }
__device__ __forceinline__ void f2_neg(F2& r, const F2& a) { f_neg(r.c0, a.c0); f_neg(r.c1, a.c1); }
__device__ __forceinline__ void f2_const(F2& r, const int32_t* k0, const int32_t* k1) { f_const(r.c0, k0); f_const(r.c1, k1); }
__device__ __forceinline__ bool f2_is_zero(const F2& a) { return f_is_zero(a.c0) && f_is_zero(a.c1); }
__device__ __forceinline__ void f_sel(Fp28& r, const Fp28& a, bool take) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = take ? a.l[i] : r.l[i];
}
__device__ __forceinline__ void f2_sel(F2& r, const F2& a, bool take) { f_sel(r.c0, a.c0, take); f_sel(r.c1, a.c1, take); }
// 1 / n = (n^((p-3)/4))^4 n, 0 for n = 0
__device__ __forceinline__ void f_inv(Fp28& r, const Fp28& n) {
    Fp28 e;
    f_pow_exp(e, n);
    f_sqr(e, e);
    f_sqr(e, e);
    f_mul(r, e, n);
}
// 1 / a = conj(a) / norm(a); a of L <= 2
__device__ __forceinline__ void f2_inv(F2& r, const F2& a) {
    Fp28 n, ni, m1;
    f_mul2(n, a.c0, a.c0, a.c1, a.c1);
    f_inv(ni, n);
    f_mul(r.c0, a.c0, ni);
    f_neg(m1, a.c1);
    f_mul(r.c1, m1, ni);
}
// y^2 = a given s, a root of norm(a): the second exponentiation of k_g2_decompress (a of L <= 2, s of L = 1)
__device__ __forceinline__ void f2_sqrt_with_norm(F2& y, const F2& a, const Fp28& s) {
    Fp28 half, t, t2, e, c, cc, h;
    f_const(half, zkp28::K28_INV2);
    f_add(t, a.c0, s);
    f_mul(t, t, half);
    f_sub(t2, a.c0, s);                  // a1 = 0 with s = -a0: t is zero, the other half is a0
    f_mul(t2, t2, half);
    f_sel(t, t2, f_is_zero(t));
    f_pow_exp(e, t);
    f_mul(c, t, e);
    f_sqr(cc, c);
    const bool c_sq = f_eq(cc, t);
    f_mul(h, a.c1, e);
    f_mul(h, h, half);
    Fp28 nh;
    f_neg(nh, h);
    y.c0 = c;
    y.c1 = h;
    f_sel(y.c0, nh, !c_sq);
    f_sel(y.c1, c, !c_sq);
}
__device__ __forceinline__ void f2_from_wire(F2& r, const uint64_t* w) {
    zkp28::fp28_from_wire(r.c0, w);
    zkp28::fp28_from_wire(r.c1, w + 6);
}
// sgn0 of RFC 9380 4.1 on canonical words
__device__ __forceinline__ uint32_t sgn0_w(const uint64_t* c0, const uint64_t* c1) { return w_is_zero(c0) ? (uint32_t)(c1[0] & 1) : (uint32_t)(c0[0] & 1); }

// a projective point in the workspace: limb k of coefficient c of coordinate v of slot s at ws[((2 v + c) 14 + k) stride + s] (a lane's
// stores are coalesced across the wavefront; k_h2c_clear's lane pairs read their own coefficient)
__device__ __forceinline__ void f_st(int32_t* ws, size_t stride, size_t slot, int at, const Fp28& a) {
#pragma unroll
    for (int i = 0; i < NL; i++) ws[(size_t)(at + i) * stride + slot] = a.l[i];
}

// ------------------------------------------------------------------------------------------- the map
// u: m field elements of Fp2 (12 words each); slot t of the workspace receives iso(sswu(u_t))
__global__ void __launch_bounds__(TPB_M) k_h2c_map(const uint64_t* u, uint32_t m, int32_t* ws, size_t stride) {
    const uint32_t t = blockIdx.x * TPB_M + threadIdx.x;
    if (t >= m) return;
    const uint64_t* uw = u + 12 * (size_t)t;
    const uint32_t sgn_u = sgn0_w(uw, uw + 6);
    F2 uu, usq, zu2, tv1, x1, gx1, k, x, a, y;
    f2_from_wire(uu, uw);
    f2_sqr(usq, uu);
    f2_const(k, zkp28::K28_SSWU_Z_0, zkp28::K28_SSWU_Z_1);
    f2_mul(zu2, k, usq);
    f2_sqr(tv1, zu2);
    f2_add(tv1, tv1, zu2);                                         // Z^2 u^4 + Z u^2: L2
    const bool exceptional = f2_is_zero(tv1);                      // u = 0 only: -1 / Z is no square
    f2_inv(x1, tv1);
    Fp28 one;
    f_const(one, zkp28::K28_ONE);
    f_add(x1.c0, x1.c0, one);
    f2_const(k, zkp28::K28_SSWU_NBA_0, zkp28::K28_SSWU_NBA_1);
    f2_mul(x1, x1, k);                                             // -B / A (1 + 1 / tv1)
    f2_const(k, zkp28::K28_SSWU_X1E_0, zkp28::K28_SSWU_X1E_1);
    f2_sel(x1, k, exceptional);                                    // B / (Z A)
    // g(x1) = (x1^2 + A) x1 + B
    f2_sqr(gx1, x1);
    f2_const(k, zkp28::K28_SSWU_A_0, zkp28::K28_SSWU_A_1);
    f2_add(gx1, gx1, k);
    f2_mul(gx1, gx1, x1);
    f2_const(k, zkp28::K28_SSWU_B_0, zkp28::K28_SSWU_B_1);
    f2_add(gx1, gx1, k);                                           // L2
    // the branch: g(x1) is a square of Fp2 iff its norm is one of Fp
    Fp28 n, s, s2, cn;
    f_mul2(n, gx1.c0, gx1.c0, gx1.c1, gx1.c1);
    const bool square = f_sqrt(s, n);                              // s^2 = n, or -n for a non-square
    // the other candidate: x2 = Z u^2 x1, g(x2) = Z^3 u^6 g(x1); norm(Z^3 g(x1)) = (s c)^2 with c^2 = -norm(Z^3)
    f2_mul(x, zu2, x1);
    f2_const(k, zkp28::K28_SSWU_Z3_0, zkp28::K28_SSWU_Z3_1);
    f2_mul(a, k, gx1);
    f_const(cn, zkp28::K28_SSWU_C_0);
    f_mul(s2, s, cn);
    f2_sel(x, x1, square);
    f2_sel(a, gx1, square);
    f_sel(s2, s, square);
    f2_sqrt_with_norm(y, a, s2);
    F2 u3, yu;
    f2_mul(u3, usq, uu);
    f2_mul(yu, y, u3);                                             // sqrt(g(x2)) = u^3 sqrt(Z^3 g(x1))
    f2_sel(y, yu, !square);
    uint64_t y0[6], y1[6];
    zkp28::fp28_to_wire(y0, y.c0);
    zkp28::fp28_to_wire(y1, y.c1);
    F2 ny;
    f2_neg(ny, y);
    f2_sel(y, ny, sgn0_w(y0, y1) != sgn_u);
    // the 3-isogeny: x_den = d^2, y_den = d^3 with d = x + 6 - 6 i; the point is (x_num d : y y_num : d^3)
    F2 d, d2, xn, yn;
    f2_const(k, zkp28::K28_ISO_DEN_0, zkp28::K28_ISO_DEN_1);
    f2_add(d, x, k);                                               // L2
    f2_sqr(d2, d);
    F2 qx, qy, qz;
    f2_mul(qz, d2, d);
    f2_const(xn, zkp28::K28_ISO_XNUM3_0, zkp28::K28_ISO_XNUM3_1);
    f2_const(yn, zkp28::K28_ISO_YNUM3_0, zkp28::K28_ISO_YNUM3_1);
    f2_mul(xn, xn, x);
    f2_mul(yn, yn, x);
    f2_const(k, zkp28::K28_ISO_XNUM2_0, zkp28::K28_ISO_XNUM2_1);
    f2_add(xn, xn, k);
    f2_mul(xn, xn, x);
    f2_const(k, zkp28::K28_ISO_YNUM2_0, zkp28::K28_ISO_YNUM2_1);
    f2_add(yn, yn, k);
    f2_mul(yn, yn, x);
    f2_const(k, zkp28::K28_ISO_XNUM1_0, zkp28::K28_ISO_XNUM1_1);
    f2_add(xn, xn, k);
    f2_mul(xn, xn, x);
    f2_const(k, zkp28::K28_ISO_YNUM1_0, zkp28::K28_ISO_YNUM1_1);
    f2_add(yn, yn, k);
    f2_mul(yn, yn, x);
    f2_const(k, zkp28::K28_ISO_XNUM0_0, zkp28::K28_ISO_XNUM0_1);
    f2_add(xn, xn, k);                                             // L2
    f2_const(k, zkp28::K28_ISO_YNUM0_0, zkp28::K28_ISO_YNUM0_1);
    f2_add(yn, yn, k);
    f2_mul(qx, xn, d);
    f2_mul(qy, y, yn);
    f_st(ws, stride, t, 0, qx.c0);
    f_st(ws, stride, t, NL, qx.c1);
    f_st(ws, stride, t, 2 * NL, qy.c0);
    f_st(ws, stride, t, 3 * NL, qy.c1);
    f_st(ws, stride, t, 4 * NL, qz.c0);
    f_st(ws, stride, t, 5 * NL, qz.c1);
}

// ------------------------------------------------------------------------------------------- the verifier's small kernels
// flag[0] = 0 (nothing refuses the batch yet); -g1 as a wire point
__global__ void k_bls_init(int* flag, uint64_t* neg_g1, uint8_t* neg_g1_inf) {
    if (blockIdx.x || threadIdx.x) return;
    flag[0] = 0;
    Fp28 x, y;
    f_const(x, zkp28::K28_G1_X);
    f_const(y, zkp28::K28_G1_Y);
    f_neg(y, y);
    zkp28::fp28_to_wire(neg_g1, x);
    zkp28::fp28_to_wire(neg_g1 + 6, y);
    *neg_g1_inf = 0;
}
// any non-zero byte (a status of the points check, an identity among the public keys) refuses the batch
// (every writer stores the same 1: a plain store, as k_rlc_fold's)
__global__ void k_bls_fold(const uint8_t* st, size_t n, int* flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && st[i]) flag[0] = 1;
}
__global__ void k_bls_finish(const int* flag, int* all_ok) {
    if (flag[0]) *all_ok = 0;
}

inline unsigned blocks_of(size_t n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

#define BLS_CHK(c, what, call)                                        \
    do {                                                              \
        if (int rc__ = ctxop::fail((c), (what), (call))) return rc__; \
    } while (0)

int tails(zkp_ctx* c, const bls::Layout& L, char* w, const void* dst, size_t dst_len, hipStream_t s) {
    hipLaunchKernelGGL(k_h2c_tails, dim3(1), dim3(1), 0, s, (const uint8_t*)dst, (uint32_t)dst_len, (uint8_t*)(w + L.tail0), (uint32_t*)(w + L.tail));
    return ctxop::fail(c, "k_h2c_tails", hipGetLastError());
}
int field_slice(zkp_ctx* c, const bls::Layout& L, char* w, const void* msgs, const void* offsets, size_t at, size_t cnt, size_t n_all, size_t dst_len,
                uint64_t* out_u, hipStream_t s) {
    hipLaunchKernelGGL(k_h2f, dim3(blocks_of(cnt, TPB_H)), dim3(TPB_H), 0, s, (const uint8_t*)msgs, (const uint64_t*)offsets, (uint64_t)at, (uint32_t)cnt,
                       (uint64_t)n_all, (const uint8_t*)(w + L.tail0), (const uint32_t*)(w + L.tail), (uint32_t)dst_len, out_u, ctxop::bls_bad_word(c));
    return ctxop::fail(c, "k_h2f", hipGetLastError());
}
// cnt <= L.slice points: u (device, cnt x 2 Fp2) through the map, the sum and the cofactor
int map_slice(zkp_ctx* c, const bls::Layout& L, char* w, const uint64_t* u, size_t cnt, uint64_t* out, uint8_t* out_inf, hipStream_t s) {
    int32_t* pts = (int32_t*)(w + L.pts);
    const size_t stride = 2 * L.slice;
    hipLaunchKernelGGL(k_h2c_map, dim3(blocks_of(2 * cnt, TPB_M)), dim3(TPB_M), 0, s, u, (uint32_t)(2 * cnt), pts, stride);
    BLS_CHK(c, "k_h2c_map", hipGetLastError());
    BLS_CHK(c, "k_h2c_clear", coop_h2c_clear(nullptr, nullptr, pts, stride, cnt, out, out_inf, s));
    return 0;
}

}  // namespace

int h2c_wide_dev(zkp_ctx* c, const void* bytes, size_t n, void* out, hipStream_t s) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_h2c_wide, dim3(blocks_of(n, TPB_H)), dim3(TPB_H), 0, s, (const uint8_t*)bytes, n, (uint64_t*)out);
    return ctxop::fail(c, "k_h2c_wide", hipGetLastError());
}

int h2c_field_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out_u, hipStream_t s) {
    if (!n) return 0;
    const bls::Layout L = bls::layout(n, false);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_bls(c, L.total, &ws)) || (rc = tails(c, L, (char*)ws, dst, dst_len, s))) return rc;
    for (size_t at = 0; at < n && !rc; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        rc = field_slice(c, L, (char*)ws, msgs, offsets, at, cnt, n, dst_len, (uint64_t*)out_u + 24 * at, s);
    }
    return rc;
}

int h2c_map_dev(zkp_ctx* c, const void* u, size_t n, void* out, void* out_inf, hipStream_t s) {
    if (!n) return 0;
    const bls::Layout L = bls::layout(n, false);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_bls(c, L.total, &ws))) return rc;
    for (size_t at = 0; at < n && !rc; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        rc = map_slice(c, L, (char*)ws, (const uint64_t*)u + 24 * at, cnt, (uint64_t*)out + 24 * at, (uint8_t*)out_inf + at, s);
    }
    return rc;
}

int h2c_clear_dev(zkp_ctx* c, const void* pts, const void* inf, size_t n, void* out, void* out_inf, hipStream_t s) {
    return ctxop::fail(c, "k_h2c_clear", coop_h2c_clear((const uint64_t*)pts, (const uint8_t*)inf, nullptr, 0, n, (uint64_t*)out, (uint8_t*)out_inf, s));
}

// the composition, slice by slice: the u values of a slice stay in the workspace
static int hash_into(zkp_ctx* c, const bls::Layout& L, char* w, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, uint64_t* out,
                     uint8_t* out_inf, hipStream_t s) {
    int rc = tails(c, L, w, dst, dst_len, s);
    uint64_t* u = (uint64_t*)(w + L.u);
    for (size_t at = 0; at < n && !rc; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        if ((rc = field_slice(c, L, w, msgs, offsets, at, cnt, n, dst_len, u, s))) break;
        rc = map_slice(c, L, w, u, cnt, out + 24 * at, out_inf + at, s);
    }
    return rc;
}

int h2c_hash_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out, void* out_inf, hipStream_t s) {
    if (!n) return 0;
    const bls::Layout L = bls::layout(n, false);
    void* ws = nullptr;
    if (int rc = ctxop::grow_bls(c, L.total, &ws)) return rc;
    return hash_into(c, L, (char*)ws, msgs, offsets, n, dst, dst_len, (uint64_t*)out, (uint8_t*)out_inf, s);
}

int bls_verify_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig,
                   const void* inf_sig, size_t n, const void* rand, int flags, int* all_ok, hipStream_t s) {
    zkp_rlc_batch b = {};
    if (!n) return rlc_check_dev(c, &b, nullptr, ZKP_RLC_POINTS_CHECKED, all_ok, s);       // the empty batch holds
    const bls::Layout L = bls::layout(n, true);
    void* ws = nullptr;
    int rc;
    if ((rc = ctxop::grow_bls(c, L.total, &ws))) return rc;
    char* w = (char*)ws;
    int* flag = (int*)(w + L.flag);
    uint64_t* hq = (uint64_t*)(w + L.hq);
    uint8_t *hinf = (uint8_t*)(w + L.hinf), *st = (uint8_t*)(w + L.st);
    hipLaunchKernelGGL(k_bls_init, dim3(1), dim3(1), 0, s, flag, (uint64_t*)(w + L.neg_g1), (uint8_t*)(w + L.neg_g1_inf));
    BLS_CHK(c, "k_bls_init", hipGetLastError());
    if (!(flags & 1)) {                                            // ZKP_BLS_POINTS_CHECKED
        if ((rc = ctxop::valid(c, 1, pk, inf_pk, n, st, s)) || (rc = ctxop::valid(c, 2, sig, inf_sig, n, st + n, s))) return rc;
        hipLaunchKernelGGL(k_bls_fold, dim3(blocks_of(2 * n, 256)), dim3(256), 0, s, (const uint8_t*)st, 2 * n, flag);
        BLS_CHK(c, "k_bls_fold", hipGetLastError());
    }
    if (inf_pk) {                                                  // KeyValidate: the identity is no public key
        hipLaunchKernelGGL(k_bls_fold, dim3(blocks_of(n, 256)), dim3(256), 0, s, (const uint8_t*)inf_pk, n, flag);
        BLS_CHK(c, "k_bls_fold", hipGetLastError());
    }
    if ((rc = hash_into(c, L, w, msgs, offsets, n, dst, dst_len, hq, hinf, s))) return rc;
    // prod_i e([r_i] pk_i, H(m_i)) e(-g1, sum_i [r_i] sig_i): one free pair per check and one column with the fixed -g1
    b.n_checks = n;
    b.k = 1;
    b.g1 = pk;
    b.g2 = hq;
    b.inf1 = inf_pk;
    b.inf2 = hinf;
    b.s1 = 1;
    b.col_g2 = sig;
    b.col_inf2 = inf_sig;
    b.fixed_g1 = w + L.neg_g1;
    b.fixed_inf1 = w + L.neg_g1_inf;
    if ((rc = rlc_check_dev(c, &b, (const uint64_t*)rand, ZKP_RLC_POINTS_CHECKED, all_ok, s))) return rc;
    hipLaunchKernelGGL(k_bls_finish, dim3(1), dim3(1), 0, s, (const int*)flag, all_ok);
    return ctxop::fail(c, "k_bls_finish", hipGetLastError());
}

#else
}  // namespace
#endif

}  // namespace zkp
