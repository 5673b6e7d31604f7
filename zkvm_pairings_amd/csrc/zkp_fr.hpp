// zkp_fr.hpp -- the BLS12-381 scalar field Fr (r = the order of G1 / G2 / Gt, 255 bits) on 8 x 32-bit Montgomery limbs (R = 2^256), and
// the exact wide accumulator of the fold sum_c w_c x_c.  Every function is __host__ __device__ and free of HIP types: zkp_groth16.hip
// and zkp_kzg.hip compile this text for gfx950 (v_mad_u64_u32 does the 32 x 32 + 64 steps), tests/test_fr_cpu.py and
// tests/test_kzg_cpu.py compile the same text with g++ and compare it with Python integers.  Further down: powers, the roots of unity
// (DERIVED like the other constants) and the per-thread pieces of the batched inversion.
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

// a host test may count the Montgomery products a routine performs: it defines this before the include
#ifndef ZKP_FR_COUNT_MUL
#define ZKP_FR_COUNT_MUL (void)0
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
    ZKP_FR_COUNT_MUL;
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


// ---- powers ------------------------------------------------------------------------------------------------------------------------
// out = a^e in Montgomery form (a and out in Montgomery form, e a plain 256-bit integer, low word first; e = 0 gives one).  Left to
// right, one bit per turn; the exponent is shifted through its eight words, so nothing is indexed by a variable.  out may alias a.
ZKP_FR_INL void mont_pow(uint32_t* out, const uint32_t* a, const uint32_t* e) {
    constexpr Consts K = make_consts();
    uint32_t base[NW], res[NW], ee[NW];
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) { base[i] = a[i]; res[i] = K.one[i]; ee[i] = e[i]; }
ZKP_FR_NOUNROLL
    for (int b = 0; b < 32 * NW; b++) {
        mont_mul(res, res, res);
        if (ee[NW - 1] >> 31) mont_mul(res, res, base);
ZKP_FR_UNROLL
        for (int w = NW - 1; w > 0; w--) ee[w] = (ee[w] << 1) | (ee[w - 1] >> 31);
        ee[0] <<= 1;
    }
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) out[i] = res[i];
}
// canonical in, canonical out
ZKP_FR_INL void pow(uint32_t* out, const uint32_t* a, const uint32_t* e) {
    uint32_t t[NW];
    to_mont(t, a);
    mont_pow(t, t, e);
    from_mont(out, t);
}
// the inverse under the Montgomery product: mont_mul(a, mont_inv(a)) = one for a != 0 mod r, and 0 for 0.  One power r - 2.
ZKP_FR_INL void mont_inv(uint32_t* out, const uint32_t* a) {
    constexpr Consts K = make_consts();
    mont_pow(out, a, K.rm2);
}

// ---- the roots of unity ------------------------------------------------------------------------------------------------------------
// r - 1 = 2^32 * odd: omega[32] = 7^((r - 1) / 2^32) generates the 2^32-point domain (the reference's FR_GENERATOR = 7, FR_S = 32,
// src/common.rs), omega[k] = omega[k + 1]^2 the 2^k-point one.  DERIVED like Consts, with a compile-time Montgomery product.
struct Roots {
    uint32_t omega[33][NW];      // Montgomery form
    uint32_t inv_pow2[33][NW];   // 2^-k mod r, Montgomery form
    uint32_t rinv[NW];           // R^-1 mod r as a plain integer: mont_mul(x, rinv) = x / R^2
};
ZKP_FR_HD constexpr void k_mont_mul(uint32_t* out, const uint32_t* a, const uint32_t* b, const Consts& k) {
    uint32_t A[NW] = {}, B[NW] = {}, t[NW + 2] = {};
    for (int i = 0; i < NW; i++) { A[i] = a[i]; B[i] = b[i]; }
    for (int i = 0; i < NW; i++) {
        uint64_t c = 0;
        for (int j = 0; j < NW; j++) {
            c += (uint64_t)A[j] * B[i] + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[NW];
        t[NW] = (uint32_t)c;
        t[NW + 1] = (uint32_t)(c >> 32);
        const uint32_t m = t[0] * k.inv;
        c = (uint64_t)m * k.r[0] + t[0];
        c >>= 32;
        for (int j = 1; j < NW; j++) {
            c += (uint64_t)m * k.r[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[NW];
        t[NW - 1] = (uint32_t)c;
        t[NW] = t[NW + 1] + (uint32_t)(c >> 32);
    }
    bool ge = t[NW] != 0;   // t >= r ?
    if (!ge) {
        ge = true;
        for (int i = NW - 1; i >= 0; i--)
            if (t[i] != k.r[i]) { ge = t[i] > k.r[i]; break; }
    }
    int64_t bw = 0;
    for (int i = 0; i < NW; i++) {
        bw += (int64_t)t[i] - (ge ? k.r[i] : 0u);
        out[i] = (uint32_t)bw;
        bw >>= 32;
    }
}
ZKP_FR_HD constexpr Roots make_roots() {
    const Consts k = make_consts();
    Roots w{};
    uint32_t g[NW] = {7, 0, 0, 0, 0, 0, 0, 0}, acc[NW] = {};
    k_mont_mul(g, g, k.r2, k);
    for (int i = 0; i < NW; i++) acc[i] = k.one[i];
    for (int wi = NW - 1; wi >= 1; wi--)          // (r - 1) >> 32 is words 1 .. 7 of r (its word 0 is 1)
        for (int b = 31; b >= 0; b--) {
            k_mont_mul(acc, acc, acc, k);
            if ((k.r[wi] >> b) & 1) k_mont_mul(acc, acc, g, k);
        }
    for (int lg = 32; lg >= 0; lg--) {
        for (int i = 0; i < NW; i++) w.omega[lg][i] = acc[i];
        k_mont_mul(acc, acc, acc, k);
    }
    for (int i = 0; i < NW; i++) acc[i] = k.one[i];
    for (int lg = 0; lg <= 32; lg++) {
        for (int i = 0; i < NW; i++) w.inv_pow2[lg][i] = acc[i];
        uint64_t c = 0;                            // acc <- acc / 2: (acc + r) / 2 for an odd acc (below 2^256: r < 2^255)
        const bool odd = acc[0] & 1;
        for (int i = 0; i < NW; i++) {
            c += (uint64_t)acc[i] + (odd ? k.r[i] : 0u);
            acc[i] = (uint32_t)c;
            c >>= 32;
        }
        for (int i = 0; i < NW; i++) acc[i] = (acc[i] >> 1) | (i + 1 < NW ? acc[i + 1] << 31 : 0u);
    }
    const uint32_t one[NW] = {1, 0, 0, 0, 0, 0, 0, 0};
    k_mont_mul(w.rinv, one, one, k);
    return w;
}

// ---- the batched inversion's per-thread pieces (Montgomery's trick; zkp_kzg.hip runs them on the device, tests/test_kzg_cpu.py on the
// host).  Canonical elements are taken AS Montgomery forms (of a / R): under mont_mul they form a group with identity `one`, and the
// inverse in it, mont_inv(a) = R^2 / a, is the canonical 1 / a after one product with rinv - which is applied once, to the inverse of
// the call's grand total, and reaches every element because the back-sweep is linear in it.
constexpr int INV_RUN = 4;        // consecutive elements of a thread
constexpr int INV_TPB = 256;      // threads of a workgroup
constexpr int INV_BLOCK = INV_RUN * INV_TPB;
// A thread's run: elements x0 .. x3 and their prefix products p1 .. p3 (p0 is x0), named one by one - nothing here is indexed by a loop
// variable, so every word stays in a register.  The back-sweep leaves the inverses in x0, p1, p2, p3.
struct InvRun {
    uint32_t x0[NW], x1[NW], x2[NW], x3[NW], p1[NW], p2[NW], p3[NW];
};
static_assert(INV_RUN == 4, "InvRun names the elements of a run");
// element j joins the run: a zero is replaced by one and noted in the mask; tot <- tot x, pj <- tot (j > 0).  One product unless j == 0.
ZKP_FR_INL void inv_fwd_step(uint32_t* xj, uint32_t* pj, uint32_t* tot, uint32_t* zero_mask, int j) {
    constexpr Consts K = make_consts();
    uint32_t nz = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) nz |= xj[i];
    if (!nz) *zero_mask |= 1u << j;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) xj[i] = nz ? xj[i] : K.one[i];
    if (j == 0) {
ZKP_FR_UNROLL
        for (int i = 0; i < NW; i++) tot[i] = xj[i];
    } else {
        mont_mul(tot, tot, xj);
ZKP_FR_UNROLL
        for (int i = 0; i < NW; i++) pj[i] = tot[i];
    }
}
// the run's m <= INV_RUN elements (canonical): p_j = x_0 ... x_j, tot = p_{m-1}, one for an empty run.  m - 1 products.
ZKP_FR_INL void inv_run_prefix(InvRun& r, uint32_t* tot, uint32_t* zero_mask, int m) {
    constexpr Consts K = make_consts();
    *zero_mask = 0;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) tot[i] = K.one[i];
    if (m > 0) inv_fwd_step(r.x0, nullptr, tot, zero_mask, 0);
    if (m > 1) inv_fwd_step(r.x1, r.p1, tot, zero_mask, 1);
    if (m > 2) inv_fwd_step(r.x2, r.p2, tot, zero_mask, 2);
    if (m > 3) inv_fwd_step(r.x3, r.p3, tot, zero_mask, 3);
}
// u = the (scaled) inverse of p_j: pj <- u p_{j-1} = the inverse of x_j (0 where the mask says so), u <- u x_j = the inverse of p_{j-1}.
// Two products; for j == 0 (pprev null) pj <- u and none.  pj may be pprev's successor only: p_j itself is no longer needed by then.
ZKP_FR_INL void inv_back_step(const uint32_t* xj, const uint32_t* pprev, uint32_t* pj, uint32_t* u, uint32_t zero_mask, int j) {
    uint32_t o[NW];
    if (pprev) {
        mont_mul(o, u, pprev);
        mont_mul(u, u, xj);
    } else {
ZKP_FR_UNROLL
        for (int i = 0; i < NW; i++) o[i] = u[i];
    }
    const bool z = (zero_mask >> j) & 1;
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) pj[i] = z ? 0u : o[i];
}
// u = the (scaled) inverse of the run's total: x0, p1, p2, p3 <- the inverses of x0 .. x3.  2 (m - 1) products.
ZKP_FR_INL void inv_run_back(InvRun& r, const uint32_t* u_in, uint32_t zero_mask, int m) {
    uint32_t u[NW];
ZKP_FR_UNROLL
    for (int i = 0; i < NW; i++) u[i] = u_in[i];
    if (m > 3) inv_back_step(r.x3, r.p2, r.p3, u, zero_mask, 3);
    if (m > 2) inv_back_step(r.x2, r.p1, r.p2, u, zero_mask, 2);
    if (m > 1) inv_back_step(r.x1, r.x0, r.p1, u, zero_mask, 1);
    if (m > 0) inv_back_step(r.x0, nullptr, r.x0, u, zero_mask, 0);
}

}  // namespace fr
}  // namespace zkp
