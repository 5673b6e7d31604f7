// zkp_bls_clear.hip -- hash-to-G2, last step (zkp_bls.hip drives it): the sum of the two mapped points and the cofactor, two lanes per point.
//
// P is the wire point i (FROM_WIRE: any point of E2, inf may be null) or the sum of the two homogeneous projective points (X : Y : Z) the
// map left in workspace slots 2 i and 2 i + 1 (limb k of coefficient c of coordinate v at ws[((2 v + c) 14 + k) stride + slot]; Z = 0 is
// the identity).  out[i] = [x^2 - x - 1] P + [x - 1] psi(P) + psi^2(2 P), x = -|x| the curve parameter, which is [h_eff] P:
//     A = [|x|] P,  B = psi(P) - A = [x] P + psi(P),  C = [|x|] B,  out = -C + A - P - psi(P) + psi^2(2 P).
// LDS slots 0..2 hold P, 3..5 A, 6..8 the base of the running ladder and then the term being added, all Jacobian; every addition is the
// full one (points of small order meet every exceptional case), one instance per loop.
//
// The arithmetic is that of zkp_coop.hip's two-lane family, restated here for Fp2 only: a lane pair holds an Fp2 value, one Fp28 per
// lane; products fetch the partner's coefficient by a DPP quad swap and travel BY VALUE through two non-inlined routines, so that the
// kernel is small and keeps everything in registers.  It is a translation unit of its own because the register allocation of
// zkp_coop.hip's kernels depends on the set of callers of those shared routines, and tests/test_fk20_cpu.py and tests/test_cells_cpu.py
// pin the register counts of that file's kernels.
#include "zkp_coop.hpp"
#include "zkp_fp28_ext.hpp"

namespace {

using namespace zkp_f28;
using zkp28::Acc;

constexpr uint64_t X_ABS = 0xd201000000010000ull;

__device__ __forceinline__ void swap_pair(Fp28& o, const Fp28& x) {
#pragma unroll
    for (int i = 0; i < NL; i++) o.l[i] = __builtin_amdgcn_update_dpp(0, x.l[i], 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, false);
}
// r = coefficient c of (a0 + a1 u)^2 :  c=0: (a0 + a1)(a0 - a1) ;  c=1: (2 a0) a1
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
    zkp28::acc_zero(acc);
    zkp28::acc_mul(acc, x, y);
    zkp28::acc_reduce(r.l, acc);
    return r;
}
// r = coefficient c of (a0 + a1 u)(b0 + b1 u) :  c=0: a0 b0 - a1 b1 ;  c=1: a0 b1 + a1 b0  (one reduction).  The second operand travels as
// four int4 vectors: an aggregate of more than 16 registers would go through the stack.
__device__ __attribute__((noinline)) Fp28 c_mul_q(Fp28 ma, int4 q0, int4 q1, int4 q2, int4 q3, int c) {
    Fp28 mb;
    mb.l[0] = q0.x; mb.l[1] = q0.y; mb.l[2] = q0.z; mb.l[3] = q0.w; mb.l[4] = q1.x; mb.l[5] = q1.y; mb.l[6] = q1.z; mb.l[7] = q1.w;
    mb.l[8] = q2.x; mb.l[9] = q2.y; mb.l[10] = q2.z; mb.l[11] = q2.w; mb.l[12] = q3.x; mb.l[13] = q3.y;
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
    zkp28::acc_zero(acc);
    zkp28::acc_mul(acc, x1, mb.l);
    zkp28::acc_mul(acc, x2, bo.l);
    zkp28::acc_reduce(r.l, acc);
    return r;
}
__device__ __forceinline__ Fp28 c_mul(const Fp28& a, const Fp28& b, int c) {
    return c_mul_q(a, make_int4(b.l[0], b.l[1], b.l[2], b.l[3]), make_int4(b.l[4], b.l[5], b.l[6], b.l[7]), make_int4(b.l[8], b.l[9], b.l[10], b.l[11]),
                   make_int4(b.l[12], b.l[13], 0, 0), c);
}
// sums carry their limbs back to |limb| <= 2^27 + 16 at once (zkp_coop.hip's f_add / f_sub): the formulas below stack up to eight of them
__device__ __forceinline__ Fp28 c_add(const Fp28& a, const Fp28& b) { Fp28 r; f_add(r, a, b); zkp28::weak_norm(r.l); return r; }
__device__ __forceinline__ Fp28 c_sub(const Fp28& a, const Fp28& b) { Fp28 r; f_sub(r, a, b); zkp28::weak_norm(r.l); return r; }
__device__ __forceinline__ Fp28 c_dbl(const Fp28& a) { Fp28 r; f_add(r, a, a); zkp28::weak_norm(r.l); return r; }
__device__ __forceinline__ Fp28 c_neg(const Fp28& a) { Fp28 r; f_neg(r, a); return r; }
__device__ __forceinline__ Fp28 c_zero() {
    Fp28 r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = 0;
    return r;
}
__device__ __forceinline__ Fp28 c_const(const int32_t* k) { Fp28 r; f_const(r, k); return r; }
// value renormalisation of a sum of a few products: q = round(top limb / p's top limb), x -= q p, one carry pass (|value| back below
// p, |limb| <= 2^27 + 16) - what the coordinates need before the next squaring
__device__ __forceinline__ Fp28 c_vred(Fp28 a) {
    const int32_t q = ((a.l[NL - 1] >> 9) * 80647 + (1 << 23)) >> 24;          // 2^33 / 80647 = 106513 = p >> 364
#pragma unroll
    for (int i = 0; i < NL; i++) a.l[i] -= q * zkp28::K28_PBAL[i];
    zkp28::weak_norm(a.l);
    return a;
}
// the Fp2 value of the lane pair is zero
__device__ __forceinline__ bool pair_is_zero(const Fp28& a) {
    const int z = f_is_zero(a) ? 1 : 0;
    const int zo = __builtin_amdgcn_update_dpp(0, z, 0xB1, 0xf, 0xf, false);
    return z && zo;
}

// values parked in LDS: limb quad q of value v at [(v * 4 + q) * 64 + lane]
__device__ __forceinline__ void park_st(int4* park, int lane, int v, const Fp28& x) {
    park[(v * 4 + 0) * 64 + lane] = make_int4(x.l[0], x.l[1], x.l[2], x.l[3]);
    park[(v * 4 + 1) * 64 + lane] = make_int4(x.l[4], x.l[5], x.l[6], x.l[7]);
    park[(v * 4 + 2) * 64 + lane] = make_int4(x.l[8], x.l[9], x.l[10], x.l[11]);
    park[(v * 4 + 3) * 64 + lane] = make_int4(x.l[12], x.l[13], 0, 0);
}
__device__ __forceinline__ Fp28 park_ld(const int4* park, int lane, int v) {
    asm volatile("" ::: "memory");   // keep the load at its use
    const int4 v0 = park[(v * 4 + 0) * 64 + lane], v1 = park[(v * 4 + 1) * 64 + lane], v2 = park[(v * 4 + 2) * 64 + lane],
               v3 = park[(v * 4 + 3) * 64 + lane];
    Fp28 x;
    x.l[0] = v0.x; x.l[1] = v0.y; x.l[2] = v0.z; x.l[3] = v0.w; x.l[4] = v1.x; x.l[5] = v1.y; x.l[6] = v1.z; x.l[7] = v1.w;
    x.l[8] = v2.x; x.l[9] = v2.y; x.l[10] = v2.z; x.l[11] = v2.w; x.l[12] = v3.x; x.l[13] = v3.y;
    return x;
}

struct Jac { Fp28 x, y, z; };   // this lane's coefficient of the Jacobian coordinates; z == 0 <=> infinity

__device__ __forceinline__ void jac_st(int4* park, int lane, int v0, const Jac& p) {
    park_st(park, lane, v0, p.x);
    park_st(park, lane, v0 + 1, p.y);
    park_st(park, lane, v0 + 2, p.z);
}
__device__ __forceinline__ Jac jac_ld(const int4* park, int lane, int v0) {
    Jac p;
    p.x = park_ld(park, lane, v0);
    p.y = park_ld(park, lane, v0 + 1);
    p.z = park_ld(park, lane, v0 + 2);
    return p;
}
// a = 0 doubling (dbl-2009-l).  Infinity and y = 0 need no special case: Z3 = 2 Y Z vanishes.
__device__ __forceinline__ void jac_dbl(Jac& p, int c) {
    Fp28 B = c_sqr(p.y, c);
    Fp28 Z3 = c_dbl(c_mul(p.y, p.z, c));
    Fp28 A = c_sqr(p.x, c);
    Fp28 t = c_sqr(c_add(p.x, B), c);
    Fp28 C = c_sqr(B, c);
    Fp28 D = c_dbl(c_sub(c_sub(t, A), C));
    Fp28 E = c_add(c_add(A, A), A);
    Fp28 X3 = c_sub(c_sub(c_sqr(E, c), D), D);
    Fp28 Y3 = c_sub(c_mul(E, c_sub(D, X3), c), c_dbl(c_dbl(c_dbl(C))));
    p.x = c_vred(X3); p.y = c_vred(Y3); p.z = c_vred(Z3);
}
// p += q, both Jacobian (add-2007-bl with Z3 = 2 Z1 Z2 H), with every exceptional case: either input at infinity, P == Q (doubled),
// P == -Q (infinity).  q = LDS slots v0 .. v0 + 2, its y negated when neg: it costs no registers across the products.
__device__ __forceinline__ void jac_add(Jac& p, const int4* park, int lane, int v0, bool neg, int c) {
    auto ldq = [&](int v) -> Fp28 {
        const Fp28 q = park_ld(park, lane, v0 + v);
        return (neg && v == 1) ? c_neg(q) : q;
    };
    if (pair_is_zero(p.z)) { p.x = ldq(0); p.y = ldq(1); p.z = ldq(2); return; }
    if (pair_is_zero(ldq(2))) return;
    Fp28 Z2 = ldq(2);
    Fp28 Z2Z2 = c_sqr(Z2, c);
    Fp28 U1 = c_mul(p.x, Z2Z2, c);
    Fp28 S1 = c_mul(p.y, c_mul(Z2, Z2Z2, c), c);
    Fp28 ZZ = c_mul(p.z, Z2, c);
    Fp28 Z1Z1 = c_sqr(p.z, c);
    Fp28 H = c_sub(c_mul(ldq(0), Z1Z1, c), U1);
    Fp28 rr = c_sub(c_mul(ldq(1), c_mul(p.z, Z1Z1, c), c), S1);
    if (pair_is_zero(H)) {
        if (pair_is_zero(rr)) { p.x = ldq(0); p.y = ldq(1); p.z = ldq(2); jac_dbl(p, c); return; }
        p.z = c_zero();   // P + (-P)
        return;
    }
    rr = c_dbl(rr);
    Fp28 I = c_sqr(c_dbl(H), c);
    Fp28 Z3 = c_mul(c_dbl(ZZ), H, c);
    Fp28 J = c_mul(H, I, c);
    Fp28 V = c_mul(U1, I, c);
    Fp28 X3 = c_sub(c_sub(c_sub(c_sqr(rr, c), J), V), V);
    Fp28 Y3 = c_sub(c_mul(rr, c_sub(V, X3), c), c_dbl(c_mul(S1, J, c)));
    p.x = c_vred(X3); p.y = c_vred(Y3); p.z = c_vred(Z3);
}

// (about 300 registers: one wavefront per SIMD; no private segment)
template <bool FROM_WIRE>
__global__ void __launch_bounds__(64) k_h2c_clear(const uint64_t* pts, const uint8_t* inf, const int32_t* ws, size_t stride, uint32_t n, uint64_t* out,
                                                  uint8_t* out_inf) {
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    const int c = (int)(tid & 1);
    uint32_t i = tid >> 1;
    const bool live = i < n;
    if (!live) i = n - 1;
    const int lane = threadIdx.x;
    __shared__ int4 park[9 * 4 * 64];
    auto conj = [&](const Fp28& v) -> Fp28 { return c ? c_neg(v) : v; };
    auto one = [&]() -> Fp28 { return c ? c_zero() : c_const(zkp28::K28_ONE); };
    auto psi = [&](Jac& t) {                                   // (conj(X) psi_x, conj(Y) psi_y, conj(Z))
        t.x = c_mul(conj(t.x), c_const(c ? zkp28::K28_PSI_X_1 : zkp28::K28_PSI_X_0), c);
        t.y = c_mul(conj(t.y), c_const(c ? zkp28::K28_PSI_Y_1 : zkp28::K28_PSI_Y_0), c);
        t.z = conj(t.z);
    };
    Jac p;
    if (FROM_WIRE) {
        zkp28::fp28_from_wire(p.x, pts + 24 * (size_t)i + 6 * c);
        zkp28::fp28_from_wire(p.y, pts + 24 * (size_t)i + 12 + 6 * c);
        p.z = one();
        if (inf && inf[i]) p.z = c_zero();
    } else {
        auto hom = [&](size_t slot) -> Jac {                  // (X : Y : Z) -> Jacobian (X Z, Y Z^2, Z)
            Fp28 v[3];
#pragma unroll
            for (int q = 0; q < 3; q++)
#pragma unroll
                for (int k = 0; k < NL; k++) v[q].l[k] = ws[(size_t)((2 * q + c) * NL + k) * stride + slot];
            Jac r;
            r.x = c_mul(v[0], v[2], c);
            r.y = c_mul(v[1], c_sqr(v[2], c), c);
            r.z = v[2];
            return r;
        };
        p = hom(2 * (size_t)i + 1);
        jac_st(park, lane, 6, p);
        p = hom(2 * (size_t)i);
        jac_add(p, park, lane, 6, false, c);
    }
    jac_st(park, lane, 0, p);
    jac_st(park, lane, 6, p);
    Jac r;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        r.x = one(); r.y = one(); r.z = c_zero();
#pragma unroll 1
        for (int b = 63; b >= 0; b--) {                        // [|x|] of slots 6..8
            jac_dbl(r, c);
            if ((X_ABS >> b) & 1) jac_add(r, park, lane, 6, false, c);
        }
        if (pass == 0) {
            jac_st(park, lane, 3, r);                          // A
            Jac t = jac_ld(park, lane, 0);
            psi(t);
            jac_add(t, park, lane, 3, true, c);
            jac_st(park, lane, 6, t);                          // B
        }
    }
    r.y = c_neg(r.y);                                          // -C
#pragma unroll 1
    for (int step = 0; step < 4; step++) {                     // + A - P - psi(P) + psi^2(2 P)
        if (step >= 2) {
            Jac t = jac_ld(park, lane, 0);
            if (step == 2) {
                psi(t);
                t.y = c_neg(t.y);
            } else {
                jac_dbl(t, c);
                psi(t);
                psi(t);
            }
            jac_st(park, lane, 6, t);
        }
        jac_add(r, park, lane, step == 0 ? 3 : (step == 1 ? 0 : 6), step == 1, c);
    }
    // to the affine wire point: 1 / (z0 + z1 u) = (z0 - z1 u) / (z0^2 + z1^2), both lanes invert the norm: 1 / n = (n^((p-3)/4))^4 n
    const bool is_inf = pair_is_zero(r.z);
    Fp28 o, nrm, e, ninv;
    swap_pair(o, r.z);
    f_mul2(nrm, r.z, r.z, o, o);
    f_pow_exp(e, nrm);
    f_sqr(e, e);
    f_sqr(e, e);
    f_mul(ninv, e, nrm);
    Fp28 zi;
    f_mul(zi, conj(r.z), ninv);
    const Fp28 zi2 = c_sqr(zi, c);
    Fp28 ax = c_mul(r.x, zi2, c), ay = c_mul(r.y, c_mul(zi2, zi, c), c);
    if (is_inf) { ax = c_zero(); ay = one(); }                 // the identity is (0, 1)
    if (live) {
        zkp28::fp28_to_wire(out + 24 * (size_t)i + 6 * c, ax);
        zkp28::fp28_to_wire(out + 24 * (size_t)i + 12 + 6 * c, ay);
        if (c == 0) out_inf[i] = is_inf ? 1 : 0;
    }
}

}  // namespace

namespace zkp {

hipError_t coop_h2c_clear(const uint64_t* pts, const uint8_t* inf, const int32_t* ws, size_t stride, size_t n, uint64_t* out, uint8_t* out_inf, hipStream_t s) {
    if (!n) return hipSuccess;
    if (pts)
        hipLaunchKernelGGL(k_h2c_clear<true>, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, s, pts, inf, ws, stride, (uint32_t)n, out, out_inf);
    else
        hipLaunchKernelGGL(k_h2c_clear<false>, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, s, pts, inf, ws, stride, (uint32_t)n, out, out_inf);
    return hipGetLastError();
}

}  // namespace zkp
