// zkp_fr.hpp -- the BLS12-381 scalar field Fr (r = the order of G1 / G2 / Gt, 255 bits) on 8 x 32-bit Montgomery limbs (R = 2^256), and
// the exact wide accumulator of the fold sum_c w_c x_c.  Every function is __host__ __device__ and free of HIP types: zkp_groth16.hip
// compiles this text for gfx950 (v_mad_u64_u32 does the 32 x 32 + 64 steps), tests/test_fr_cpu.py compiles the same text with g++ and
// compares it with Python integers.
//
// What each function stands in for in the reference (paths relative to /root/reference):
//   add :402-411, sub :384-398, neg :415-431, mul :365-381 (a BigUint product and remainder there, a Montgomery product here),
//   square :225-227, invert :266-362 (the same power r - 2, by plain square-and-multiply), from_bytes_wide / from_u512 :192-217
//   (d0 R^2 + d1 R^3 in Montgomery form there; reduce_wide below does the same with one more word on top).
// At the wire an element is uint64_t[4], little-endian, canonical (< r): wire_load / wire_store / is_canonical.
//
// The constants are DERIVED, at compile time, from the one literal r: R mod r, R^2, R^3, R^4 by repeated doubling, -r^-1 mod 2^32 by
// Newton's iteration, r - 2 by subtraction.  The CPU gate checks each against pow / % on Python integers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZKP_FR_HD __host__ __device__
#define ZKP_FR_INL __host__ __device__ __forceinline__   // the constants are locals: they fold into immediates only once inlined
#define ZKP_FR_UNROLL _Pragma("unroll")
#define ZKP_FR_NOUNROLL _Pragma("unroll 1")
#else
#define ZKP_FR_HD
#define ZKP_FR_INL inline
#define ZKP_FR_UNROLL
#define ZKP_FR_NOUNROLL
#endif

namespace zkp {
namespace fr {

constexpr int NW = 8;          // 32-bit words of an element
constexpr int ACC_WORDS = 17;  // the fold's accumulator: 544 bits, see acc_mad

struct Consts {
    uint32_t r[NW];       // the modulus
    uint32_t rm2[NW];     // r - 2, the inversion exponent
    uint32_t one[NW];     // R mod r = the Montgomery form of 1
    uint32_t r2[NW];      // R^2 mod r
    uint32_t r3[NW];      // R^3 mod r
    uint32_t r4[NW];      // R^4 mod r
    uint32_t inv;         // -r^-1 mod 2^32
};

// a <- 2 a mod r for a < r (r < 2^255: 2 a has no carry out of 256 bits)
ZKP_FR_HD constexpr void k_double(uint32_t* a, const uint32_t* r) {
    uint32_t c = 0;
    for (int i = 0; i < NW; i++) {
        const uint32_t v = a[i];
        a[i] = (v << 1) | c;
        c = v >> 31;
    }
    bool ge = true;   // a >= r ?
    for (int i = NW - 1; i >= 0; i--)
        if (a[i] != r[i]) { ge = a[i] > r[i]; break; }
    if (ge) {
        int64_t bw = 0;
        for (int i = 0; i < NW; i++) {
            bw += (int64_t)a[i] - r[i];
            a[i] = (uint32_t)bw;
            bw >>= 32;
        }
    }
}

ZKP_FR_HD constexpr Consts make_consts() {
    // r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001 (the BLS12-381 group order), low word first
    const uint64_t r64[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
    Consts k{};
    for (int i = 0; i < 4; i++) {
        k.r[2 * i] = (uint32_t)r64[i];
        k.r[2 * i + 1] = (uint32_t)(r64[i] >> 32);
    }
    int64_t bw = -2;
    for (int i = 0; i < NW; i++) {
        bw += (int64_t)k.r[i];
        k.rm2[i] = (uint32_t)bw;
        bw >>= 32;
    }
    uint32_t t[NW] = {1, 0, 0, 0, 0, 0, 0, 0};
    for (int p = 1; p <= 4; p++) {
        for (int i = 0; i < 256; i++) k_double(t, k.r);   // t = R^p mod r
        uint32_t* dst = p == 1 ? k.one : p == 2 ? k.r2 : p == 3 ? k.r3 : k.r4;
        for (int i = 0; i < NW; i++) dst[i] = t[i];
    }
    uint32_t x = 1;   // x = r^-1 mod 2^32: each step doubles the number of correct low bits (r is odd: 1 bit to start with)
    for (int i = 0; i < 5; i++) x *= 2u - k.r[0] * x;
    k.inv = 0u - x;
    return k;
}

// ---- canonical elements -------------------------------------------------------------------------------------------------------
ZKP_FR_INL void wire_load(uint32_t* a, const uint64_t* src) {
ZKP_FR_UNROLL
    for (int i = 0; i < 4; i++) {
        a[2 * i] = (uint32_t)src[i];
        a[2 * i + 1] = (uint32_t)(src[i] >> 32);
    }
}
ZKP_FR_INL void wire_store(uint64_t* dst, const uint32_t* a) {
ZKP_FR_UNROLL
    for (int i = 0; i < 4; i++) dst[i] = (uint64_t)a[2 * i] | ((uint64_t)a[2 * i + 1] << 32);
}
// a < r
ZKP_FR_INL bool is_canonical(const uint32_t* a) {
    constexpr Consts K = make_consts();
    int64_t bw = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) {
        bw += (int64_t)a[i] - K.r[i];
        bw >>= 32;
    }
    return bw != 0;   // the subtraction borrowed
}
// t (9 words, below 2 r) -> out = t mod r
ZKP_FR_INL void cond_sub(uint32_t* out, const uint32_t* t) {
    constexpr Consts K = make_consts();
    uint32_t d[NW];
    int64_t bw = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) {
        bw += (int64_t)t[i] - K.r[i];
        d[i] = (uint32_t)bw;
        bw >>= 32;
    }
    bw += (int64_t)t[NW];
    const bool keep = bw < 0;   // t < r
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) out[i] = keep ? t[i] : d[i];
}
ZKP_FR_INL void add(uint32_t* out, const uint32_t* a, const uint32_t* b) {
    uint32_t t[NW + 1];
    uint64_t c = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) {
        c += (uint64_t)a[i] + b[i];
        t[i] = (uint32_t)c;
        c >>= 32;
    }
    t[NW] = (uint32_t)c;
    cond_sub(out, t);
}
ZKP_FR_INL void sub(uint32_t* out, const uint32_t* a, const uint32_t* b) {
    constexpr Consts K = make_consts();
    uint32_t d[NW];
    int64_t bw = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) {
        bw += (int64_t)a[i] - b[i];
        d[i] = (uint32_t)bw;
        bw >>= 32;
    }
    const uint32_t mask = bw != 0 ? 0xffffffffu : 0u;
    uint64_t c = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) {
        c += (uint64_t)d[i] + (K.r[i] & mask);
        out[i] = (uint32_t)c;
        c >>= 32;
    }
}
ZKP_FR_INL void neg(uint32_t* out, const uint32_t* a) {
    const uint32_t z[NW] = {0, 0, 0, 0, 0, 0, 0, 0};
    sub(out, z, a);
}

// ---- Montgomery product: out = a b / R mod r, for a < 2^256 and b < r (the result is below 2 r before the last subtraction).  CIOS on
// 32-bit words; out may alias a or b.
ZKP_FR_INL void mont_mul(uint32_t* out, const uint32_t* a, const uint32_t* b) {
    constexpr Consts K = make_consts();
    uint32_t A[NW], B[NW], t[NW + 2];
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) { A[i] = a[i]; B[i] = b[i]; t[i] = 0; }
    t[NW] = t[NW + 1] = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) {
        uint64_t c = 0;
ZKP_FR_UNROLL
        for (int j = 0; j < NW; j++) {
            c += (uint64_t)A[j] * B[i] + t[j];   // (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1: no overflow
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[NW];
        t[NW] = (uint32_t)c;
        t[NW + 1] = (uint32_t)(c >> 32);
        const uint32_t m = t[0] * K.inv;
        c = (uint64_t)m * K.r[0] + t[0];
        c >>= 32;
ZKP_FR_UNROLL
        for (int j = 1; j < NW; j++) {
            c += (uint64_t)m * K.r[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[NW];
        t[NW - 1] = (uint32_t)c;
        t[NW] = t[NW + 1] + (uint32_t)(c >> 32);
    }
    cond_sub(out, t);
}
ZKP_FR_INL void to_mont(uint32_t* out, const uint32_t* a) {
    constexpr Consts K = make_consts();
    mont_mul(out, a, K.r2);
}
ZKP_FR_INL void from_mont(uint32_t* out, const uint32_t* a) {
    const uint32_t one[NW] = {1, 0, 0, 0, 0, 0, 0, 0};
    mont_mul(out, a, one);
}
// canonical in, canonical out: (a b / R) R^2 / R
ZKP_FR_INL void mul(uint32_t* out, const uint32_t* a, const uint32_t* b) {
    uint32_t t[NW];
    mont_mul(t, a, b);
    to_mont(out, t);
}
// a^(r - 2): the inverse, and 0 for 0 (the reference returns None there)
ZKP_FR_INL void invert(uint32_t* out, const uint32_t* a) {
    constexpr Consts K = make_consts();
    uint32_t base[NW], res[NW];
    to_mont(base, a);
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) res[i] = K.one[i];
ZKP_FR_UNROLL
    for (int w = NW - 1; w >= 0; w--) {
        const uint32_t e = K.rm2[w];
ZKP_FR_NOUNROLL
        for (int b = 31; b >= 0; b--) {
            mont_mul(res, res, res);
            if ((e >> b) & 1) mont_mul(res, res, base);
        }
    }
    from_mont(out, res);
}

// ---- the wide accumulator ----------------------------------------------------------------------------------------------------------
// acc += w x as plain integers.  Bound: w, x < 2^256 (canonical ones < r < 2^255), so a product is below 2^512 (r^2 < 2^510); a sum of
// at most 2^24 of them is below 2^536 (2^534 for canonical operands) < 2^544 = 17 words: the accumulator cannot overflow, and sums of
// such accumulators over disjoint terms cannot either.  No reduction here: reduce_wide runs once per output.
ZKP_FR_INL void acc_mad(uint32_t* acc, const uint32_t* w, const uint32_t* x) {
    uint32_t p[2 * NW];
ZKP_FR_UNROLL
    for (int i = 0; i < 2 * NW; i++) p[i] = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) {
        uint64_t c = 0;
ZKP_FR_UNROLL
        for (int j = 0; j < NW; j++) {
            c += (uint64_t)w[i] * x[j] + p[i + j];
            p[i + j] = (uint32_t)c;
            c >>= 32;
        }
        p[i + NW] = (uint32_t)c;
    }
    uint64_t c = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < 2 * NW; i++) {
        c += (uint64_t)acc[i] + p[i];
        acc[i] = (uint32_t)c;
        c >>= 32;
    }
    acc[2 * NW] += (uint32_t)c;
}
// acc += v, v of nv words (nv <= ACC_WORDS)
ZKP_FR_INL void acc_add(uint32_t* acc, const uint32_t* v, int nv) {
    uint64_t c = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < ACC_WORDS; i++) {
        c += (uint64_t)acc[i] + (i < nv ? v[i] : 0u);
        acc[i] = (uint32_t)c;
        c >>= 32;
    }
}
// out = v mod r for a 17-word integer v = lo + 2^256 mid + 2^512 top: lo R + mid R^2 + top R^3 is its Montgomery form (three products
// with R^2, R^3, R^4), one more product with 1 leaves it.  With top = 0 this is from_u512.
ZKP_FR_INL void reduce_wide(uint32_t* out, const uint32_t* v) {
    constexpr Consts K = make_consts();
    uint32_t a[NW], b[NW], t[NW];
    mont_mul(a, v, K.r2);
    mont_mul(b, v + NW, K.r3);
    add(a, a, b);
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) t[i] = i == 0 ? v[2 * NW] : 0u;
    mont_mul(b, t, K.r4);
    add(a, a, b);
    from_mont(out, a);
}

}  // namespace fr
}  // namespace zkp
