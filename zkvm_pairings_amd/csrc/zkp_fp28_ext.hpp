// zkp_fp28_ext.hpp -- what the one-element-per-lane kernels on the 28-bit core share (zkp_compress.hip, zkp_bls.hip): limb-wise Fp
// helpers over zkp_fp28.hpp's mont_mul_ps, the fixed exponentiation x^((p-3)/4) behind both square roots and the inversion, and Fp2.
// Everything is force-inlined and register-resident: no kernel that uses it has a private segment.
#pragma once
#include "zkp_fp28.hpp"

namespace zkp_f28 {

using zkp28::Fp28;
using zkp28::NL;

// canonical 6 x u64 little-endian wire constants
__device__ __constant__ const uint64_t KW_P[6] = {0xb9feffffffffaaabull, 0x1eabfffeb153ffffull, 0x6730d2a0f6b0f624ull,
                                                  0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull, 0x1a0111ea397fe69aull};
// (p-3)/4 (src/fp2.rs:238-245; (p+1)/4 of src/fp.rs:287-294 is this + 1)
__device__ __constant__ const uint64_t KW_EXP[6] = {0xee7fbfffffffeaaaull, 0x07aaffffac54ffffull, 0xd9cc34a83dac3d89ull,
                                                    0xd91dd2e13ce144afull, 0x92c6e9ed90d2eb35ull, 0x0680447a8e5ff9a6ull};
// (p-1)/2: the largest "small" y of the sign rule, and the exponent of src/fp2.rs:259-266
__device__ __constant__ const uint64_t KW_HALF[6] = {0xdcff7fffffffd555ull, 0x0f55ffff58a9ffffull, 0xb39869507b587b12ull,
                                                     0xb23ba5c279c2895full, 0x258dd3db21a5d66bull, 0x0d0088f51cbff34dull};
// (p+1)/2 = 1/2 mod p
__device__ __constant__ const uint64_t KW_INV2[6] = {0xdcff7fffffffd556ull, 0x0f55ffff58a9ffffull, 0xb39869507b587b12ull,
                                                     0xb23ba5c279c2895full, 0x258dd3db21a5d66bull, 0x0d0088f51cbff34dull};
constexpr int EXP_TOP = 378;   // top set bit of (p-3)/4
constexpr int WIN = 4;         // sliding window width: 2^(WIN-1) odd powers in the table

// ------------------------------------------------------------------------------------------- Fp (28-bit core)
__device__ __forceinline__ void f_mul(Fp28& r, const Fp28& a, const Fp28& b) {
    Fp28 t;
    zkp28::mont_mul_ps<false>(t.l, a.l, b.l, nullptr, nullptr);
    r = t;
}
// r = a0 b0 + a1 b1 (one reduction)
__device__ __forceinline__ void f_mul2(Fp28& r, const Fp28& a0, const Fp28& b0, const Fp28& a1, const Fp28& b1) {
    Fp28 t;
    zkp28::mont_mul_ps<true>(t.l, a0.l, b0.l, a1.l, b1.l);
    r = t;
}
__device__ __forceinline__ void f_sqr(Fp28& r, const Fp28& a) { f_mul(r, a, a); }
// limb-wise: the results stay within the bounds mont_mul_ps takes (|limb| < 2^29, |value| < 8p) when the inputs are products
__device__ __forceinline__ void f_add(Fp28& r, const Fp28& a, const Fp28& b) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = a.l[i] + b.l[i];
}
__device__ __forceinline__ void f_sub(Fp28& r, const Fp28& a, const Fp28& b) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = a.l[i] - b.l[i];
}
__device__ __forceinline__ void f_neg(Fp28& r, const Fp28& a) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = -a.l[i];
}
__device__ __forceinline__ void f_const(Fp28& r, const int32_t* k) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = k[i];
}
__device__ __forceinline__ void f_from_const(Fp28& r, const uint64_t* k) {
    uint64_t w[6];
#pragma unroll
    for (int i = 0; i < 6; i++) w[i] = k[i];
    zkp28::fp28_from_wire(r, w);
}
__device__ __forceinline__ bool w_is_zero(const uint64_t* a) { return (a[0] | a[1] | a[2] | a[3] | a[4] | a[5]) == 0; }
__device__ __forceinline__ bool w_eq(const uint64_t* a, const uint64_t* b) {
    uint64_t d = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) d |= a[i] ^ b[i];
    return d == 0;
}
__device__ __forceinline__ bool f_eq(const Fp28& a, const Fp28& b) {
    uint64_t x[6], y[6];
    zkp28::fp28_to_wire(x, a);
    zkp28::fp28_to_wire(y, b);
    return w_eq(x, y);
}
__device__ __forceinline__ bool f_is_zero(const Fp28& a) {
    uint64_t x[6];
    zkp28::fp28_to_wire(x, a);
    return w_is_zero(x);
}
// r = take ? a : r, as v_cndmask_b32 on the ballot of `take` (uniform where it is used).  Written in asm so that the compiler cannot turn a
// chain of these selects over the window table back into a dynamically indexed (scratch) array.
#ifdef ZKP_FP28_HOST   // the host builds of the tests: the same select in plain C++
__device__ __forceinline__ void f_select(Fp28& r, const Fp28& a, bool take) {
    for (int i = 0; i < NL; i++) r.l[i] = take ? a.l[i] : r.l[i];
}
#else
__device__ __forceinline__ void f_select(Fp28& r, const Fp28& a, bool take) {
    const uint64_t m = __builtin_amdgcn_ballot_w64(take);   // an SGPR pair: the lanes that take a
#pragma unroll
    for (int i = 0; i < NL; i++) {
        int32_t v;
        asm volatile("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(v) : "v"(r.l[i]), "v"(a.l[i]), "s"(m));
        r.l[i] = v;
    }
}
#endif
__device__ __forceinline__ bool e_bit(int i) { return (KW_EXP[i >> 6] >> (i & 63)) & 1; }

// r = a^((p-3)/4): left-to-right sliding window over the odd powers a^1 .. a^(2^WIN - 1).  The exponent and so the whole schedule
// (zero runs, window ends, digits) are uniform: the bit scan runs on scalar registers, and the digit picks its table entry by
// f_select over eight named values - the table never leaves the register file (no scratch).
__device__ __forceinline__ void f_pow_exp(Fp28& r, const Fp28& a) {
    static_assert(WIN == 4, "the table below holds 2^(WIN-1) = 8 odd powers");
    Fp28 a2, t1, t3, t5, t7, t9, t11, t13, t15;   // named, not an array: nothing about the table can become an indexed access
    f_sqr(a2, a);
    t1 = a;
    f_mul(t3, t1, a2);
    f_mul(t5, t3, a2);
    f_mul(t7, t5, a2);
    f_mul(t9, t7, a2);
    f_mul(t11, t9, a2);
    f_mul(t13, t11, a2);
    f_mul(t15, t13, a2);
    bool first = true;
    int i = EXP_TOP;
    while (i >= 0) {
        if (!e_bit(i)) {
            f_sqr(r, r);
            i--;
            continue;
        }
        int j = i - WIN + 1 < 0 ? 0 : i - WIN + 1;
        while (!e_bit(j)) j++;
        int d = 0;
        for (int b = i; b >= j; b--) d = 2 * d + (e_bit(b) ? 1 : 0);
        Fp28 t = t1;
        f_select(t, t3, d == 3);
        f_select(t, t5, d == 5);
        f_select(t, t7, d == 7);
        f_select(t, t9, d == 9);
        f_select(t, t11, d == 11);
        f_select(t, t13, d == 13);
        f_select(t, t15, d == 15);
        if (first) {
            r = t;
            first = false;
        } else {
            for (int b = i; b >= j; b--) f_sqr(r, r);
            f_mul(r, r, t);
        }
        i = j - 1;
    }
}
// *root = a^((p+1)/4); returns root^2 == a (Fp::sqrt, src/fp.rs:280-300)
__device__ __forceinline__ bool f_sqrt(Fp28& root, const Fp28& a) {
    Fp28 u, c;
    f_pow_exp(u, a);
    f_mul(root, u, a);
    f_sqr(c, root);
    return f_eq(c, a);
}

// ------------------------------------------------------------------------------------------- Fp2
struct F2 { Fp28 c0, c1; };
__device__ __forceinline__ void f2_mul(F2& r, const F2& a, const F2& b) {
    Fp28 nb1, c0, c1;
    f_neg(nb1, b.c1);
    f_mul2(c0, a.c0, b.c0, a.c1, nb1);
    f_mul2(c1, a.c0, b.c1, a.c1, b.c0);
    r.c0 = c0;
    r.c1 = c1;
}
__device__ __forceinline__ void f2_sqr(F2& r, const F2& a) {
    Fp28 s, d, t, c0, c1;
    f_add(s, a.c0, a.c1);
    f_sub(d, a.c0, a.c1);
    f_add(t, a.c0, a.c0);
    f_mul(c0, s, d);
    f_mul(c1, t, a.c1);
    r.c0 = c0;
    r.c1 = c1;
}
__device__ __forceinline__ bool f2_eq(const F2& a, const F2& b) { return f_eq(a.c0, b.c0) && f_eq(a.c1, b.c1); }
__device__ __forceinline__ void f2_one(F2& r) {
    f_const(r.c0, zkp28::K28_ONE);
#pragma unroll
    for (int i = 0; i < NL; i++) r.c1.l[i] = 0;
}
// square-and-multiply over a 384-bit exponent in constant memory (the reference's pow_vartime, src/fp2.rs:301-313; same value)
__device__ __forceinline__ void f2_pow(F2& r, const F2& a, const uint64_t* e) {
    F2 res;
    f2_one(res);
    for (int i = 383; i >= 0; i--) {
        f2_sqr(res, res);
        if ((e[i >> 6] >> (i & 63)) & 1) f2_mul(res, res, a);
    }
    r = res;
}

}  // namespace zkp_f28
