// zkp_compress.hip -- compressed BLS12-381 points on the GPU (gfx950): the square roots of Fp and Fp2, the compressed point codec
// (48 B per G1 point, 96 B per G2 point) and the square-root hooks of the C ABI.
//
// What each kernel stands in for (paths relative to the reference crate):
//   k_fp_sqrt        Fp::sqrt, src/fp.rs:280-300: a^((p+1)/4), checked by squaring
//   k_fp2_sqrt       Fp2::sqrt, src/fp2.rs:231-273, step for step (the alpha == -1 branch included): bit-exact root
//   k_g*_decompress  the usual compressed serialisation (flags 0x80 compressed, 0x40 infinity, 0x20 sort = y is the larger of
//                    y and -y); x^3 + b -> any square root -> the sign the sort flag selects.  No subgroup check (is_valid does that).
//   k_g*_compress    x and the sign of y only: no field arithmetic, no assumption that the point is valid
//
// Arithmetic: the 14 x 28-bit carry-free core of zkp_fp28.hpp (mont_mul_ps: one product per call, every operand in registers,
// force-inlined - nothing passes through memory, so no kernel here has a private segment).  Comparisons convert to canonical
// wire limbs (fp28_to_wire) first.
//
// Cost model, per element (one product = one mont_mul_ps):
//   x^((p-3)/4): the exponent has 379 bits, 228 of them set.  Square-and-multiply costs 606 products; a sliding window of 4 bits
//   over a table of the odd powers a, a^3 .. a^15 (8 entries, 112 registers, selected by the window's uniform digit) costs
//   375 squares + 78 products + 8 for the table = 461.  (p+1)/4 = (p-3)/4 + 1 is one more product, so both roots share it.
//   G1 decompression: one exponentiation (x^3 + 4)^((p+1)/4) + 5 products.
//   G2 decompression: two Fp exponentiations and no inversion - the norm's root s = N^((p+1)/4) with N = a0^2 + a1^2, then
//   t = (a0 + s)/2 and e = t^((p-3)/4): c = t e has c^2 = +-t and 1/c = +-e with the same sign, so
//   y = (c, a1 e/2) if c^2 = t, else (-a1 e/2, c).  a1 = 0 takes sqrt(a0) or u sqrt(-a0) from the same two exponentiations.
#include "zkp_compress.hpp"
#include "zkp_fp28_ext.hpp"

namespace {

using namespace zkp_f28;

constexpr int TPB_C = 256;


// ------------------------------------------------------------------------------------------- wire helpers
__device__ __forceinline__ bool w_lt_p(const uint64_t* a) {
    // a < p  <=>  a - p borrows
    bool borrow = false;
#pragma unroll
    for (int i = 0; i < 6; i++) borrow = a[i] < KW_P[i] || (a[i] == KW_P[i] && borrow);
    return borrow;
}
// a > (p-1)/2 on canonical limbs: the lexicographically larger of y and -y
__device__ __forceinline__ bool w_gt_half(const uint64_t* a) {
    int r = 0;
#pragma unroll
    for (int i = 5; i >= 0; i--)
        if (r == 0) r = a[i] > KW_HALF[i] ? 1 : (a[i] < KW_HALF[i] ? -1 : 0);
    return r > 0;
}
// a = -a on canonical limbs (0 stays 0)
__device__ __forceinline__ void w_neg(uint64_t* a) {
    if (w_is_zero(a)) return;
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const uint64_t p = KW_P[i];
        const uint64_t d0 = p - a[i];
        const uint64_t b1 = p < a[i];
        const uint64_t d = d0 - borrow;
        const uint64_t b2 = d0 < borrow;
        a[i] = d;
        borrow = b1 | b2;
    }
}

template <bool ALIGNED>
__device__ __forceinline__ uint64_t be64_load(const uint8_t* p) {
    if (ALIGNED) return __builtin_bswap64(*reinterpret_cast<const uint64_t*>(p));
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) v = (v << 8) | p[b];
    return v;
}
template <bool ALIGNED>
__device__ __forceinline__ void be64_store(uint8_t* p, uint64_t v) {
    if (ALIGNED) {
        *reinterpret_cast<uint64_t*>(p) = __builtin_bswap64(v);
    } else {
        for (int b = 0; b < 8; b++) p[b] = (uint8_t)(v >> (56 - 8 * b));
    }
}
// one big-endian 48-byte field element -> 6 LE words (flag bits of the first element stripped by the caller)
template <bool ALIGNED>
__device__ __forceinline__ void read_fe(uint64_t* w, const uint8_t* src) {
#pragma unroll
    for (int k = 0; k < 6; k++) w[5 - k] = be64_load<ALIGNED>(src + 8 * k);
}
template <bool ALIGNED>
__device__ __forceinline__ void write_fe(uint8_t* dst, const uint64_t* w, uint64_t top_flags) {
#pragma unroll
    for (int k = 0; k < 6; k++) be64_store<ALIGNED>(dst + 8 * k, w[5 - k] | (k == 0 ? top_flags : 0));
}
constexpr uint64_t FLAG_MASK = 0x1fffffffffffffffull;
constexpr uint64_t F_COMPRESSED = 0x8000000000000000ull, F_INFINITY = 0x4000000000000000ull, F_SORT = 0x2000000000000000ull;

// flags of a compressed string: 0 ok (finite), 2 malformed; *inf for a well-formed infinity
__device__ __forceinline__ uint8_t flag_status(uint8_t flags, bool rest_zero, bool* inf) {
    *inf = false;
    if (!(flags & 0x80)) return 2;
    if (flags & 0x40) {
        if ((flags & 0x20) || !rest_zero) return 2;
        *inf = true;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------- kernels
__global__ void __launch_bounds__(TPB_C) k_fp_sqrt(const uint64_t* a, size_t n, uint64_t* out, uint8_t* is_sq) {
    const size_t i = (size_t)blockIdx.x * TPB_C + threadIdx.x;
    if (i >= n) return;
    Fp28 x, s;
    zkp28::fp28_from_wire(x, a + 6 * i);
    const bool ok = f_sqrt(s, x);
    uint64_t w[6];
    zkp28::fp28_to_wire(w, s);
#pragma unroll
    for (int k = 0; k < 6; k++) out[6 * i + k] = ok ? w[k] : 0;
    is_sq[i] = ok ? 1 : 0;
}

// Fp2::sqrt of src/fp2.rs:231-273 step for step
__global__ void __launch_bounds__(TPB_C) k_fp2_sqrt(const uint64_t* a, size_t n, uint64_t* out, uint8_t* is_sq) {
    const size_t i = (size_t)blockIdx.x * TPB_C + threadIdx.x;
    if (i >= n) return;
    const uint64_t* src = a + 12 * i;
    uint64_t w0[6], w1[6];
    bool ok = true;
    if (w_is_zero(src) && w_is_zero(src + 6)) {
#pragma unroll
        for (int k = 0; k < 6; k++) w0[k] = w1[k] = 0;
    } else {
        F2 x, a1, alpha, x0, t, one;
        zkp28::fp28_from_wire(x.c0, src);
        zkp28::fp28_from_wire(x.c1, src + 6);
        f2_pow(a1, x, KW_EXP);           // a1 = self^((p-3)/4)
        f2_sqr(alpha, a1);
        f2_mul(alpha, alpha, x);         // alpha = a1^2 * self
        f2_mul(x0, a1, x);               // x0 = self^((p+1)/4)
        zkp28::fp28_to_wire(w0, alpha.c0);
        zkp28::fp28_to_wire(w1, alpha.c1);
        uint64_t m1[6];
#pragma unroll
        for (int k = 0; k < 6; k++) m1[k] = KW_P[k];
        m1[0] -= 1;
        if (w_eq(w0, m1) && w_is_zero(w1)) {          // alpha == -1: the root is x0 * u
            Fp28 nc1;
            f_neg(nc1, x0.c1);
            zkp28::fp28_to_wire(w0, nc1);
            zkp28::fp28_to_wire(w1, x0.c0);
        } else {                                       // (1 + alpha)^((p-1)/2) * x0, kept only if it squares back to self
            f2_one(one);
            f_add(alpha.c0, alpha.c0, one.c0);
            f2_pow(t, alpha, KW_HALF);
            f2_mul(t, t, x0);
            F2 chk;
            f2_sqr(chk, t);
            ok = f2_eq(chk, x);
            zkp28::fp28_to_wire(w0, t.c0);
            zkp28::fp28_to_wire(w1, t.c1);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        out[12 * i + k] = ok ? w0[k] : 0;
        out[12 * i + 6 + k] = ok ? w1[k] : 0;
    }
    is_sq[i] = ok ? 1 : 0;
}

// 48 bytes -> (x, y) + infinity byte + status (0 ok, 1 x >= p, 2 malformed, 3 x^3 + 4 is not a square)
template <bool ALIGNED>
__global__ void __launch_bounds__(TPB_C) k_g1_decompress(const uint8_t* bytes, size_t n, uint64_t* out, uint8_t* out_inf, uint8_t* status) {
    const size_t i = (size_t)blockIdx.x * TPB_C + threadIdx.x;
    if (i >= n) return;
    const uint8_t* src = bytes + 48 * i;
    uint64_t x[6], y[6] = {0, 0, 0, 0, 0, 0};
    read_fe<ALIGNED>(x, src);
    const uint8_t flags = (uint8_t)(x[5] >> 56) & 0xe0;
    x[5] &= FLAG_MASK;
    bool inf;
    uint8_t st = flag_status(flags, w_is_zero(x), &inf);
    if (!st && !inf && !w_lt_p(x)) st = 1;
    if (!st && !inf) {
        Fp28 fx, rhs, b, r;
        zkp28::fp28_from_wire(fx, x);
        f_sqr(rhs, fx);
        f_mul(rhs, rhs, fx);
        f_const(b, zkp28::K28_B);
        f_add(rhs, rhs, b);
        if (!f_sqrt(r, rhs)) {
            st = 3;
        } else {
            zkp28::fp28_to_wire(y, r);
            if (w_gt_half(y) != ((flags & 0x20) != 0)) w_neg(y);
        }
    }
    const bool zero = st || inf;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        out[12 * i + k] = zero ? 0 : x[k];
        out[12 * i + 6 + k] = zero ? 0 : y[k];
    }
    if (inf && !st) out[12 * i + 6] = 1;   // identity is (0, 1), as the uncompressed decode gives it
    out_inf[i] = inf && !st;
    status[i] = st;
}

// 96 bytes (x.c1 | x.c0) -> (x, y) + infinity byte + status (0 ok, 1 x.c0 or x.c1 >= p, 2 malformed, 3 x^3 + 4(1+u) not a square)
template <bool ALIGNED>
__global__ void __launch_bounds__(TPB_C) k_g2_decompress(const uint8_t* bytes, size_t n, uint64_t* out, uint8_t* out_inf, uint8_t* status) {
    const size_t i = (size_t)blockIdx.x * TPB_C + threadIdx.x;
    if (i >= n) return;
    const uint8_t* src = bytes + 96 * i;
    uint64_t x0[6], x1[6], y0[6] = {0, 0, 0, 0, 0, 0}, y1[6] = {0, 0, 0, 0, 0, 0};
    read_fe<ALIGNED>(x1, src);
    read_fe<ALIGNED>(x0, src + 48);
    const uint8_t flags = (uint8_t)(x1[5] >> 56) & 0xe0;
    x1[5] &= FLAG_MASK;
    bool inf;
    uint8_t st = flag_status(flags, w_is_zero(x0) && w_is_zero(x1), &inf);
    if (!st && !inf && !(w_lt_p(x0) && w_lt_p(x1))) st = 1;
    if (!st && !inf) {
        F2 x, a, x2;
        zkp28::fp28_from_wire(x.c0, x0);
        zkp28::fp28_from_wire(x.c1, x1);
        f2_sqr(x2, x);
        f2_mul(a, x2, x);
        Fp28 b, half;
        f_const(b, zkp28::K28_B);
        f_add(a.c0, a.c0, b);
        f_add(a.c1, a.c1, b);
        f_from_const(half, KW_INV2);
        // a = a0 + a1 u;  first exponentiation: sqrt(a0) when a1 == 0, else sqrt(N), N = a0^2 + a1^2
        const bool a1z = f_is_zero(a.c1);
        Fp28 base1, s;
        if (a1z) base1 = a.c0;
        else f_mul2(base1, a.c0, a.c0, a.c1, a.c1);
        const bool ok1 = f_sqrt(s, base1);
        // second: t^((p-3)/4) with t = (a0 + s)/2, or sqrt(-a0) when a1 == 0
        Fp28 base2, e, c, cc;
        if (a1z) {
            f_neg(base2, a.c0);
        } else {
            Fp28 t;
            f_add(t, a.c0, s);
            f_mul(base2, t, half);
        }
        f_pow_exp(e, base2);
        f_mul(c, base2, e);
        f_sqr(cc, c);
        const bool c_sq = f_eq(cc, base2);
        F2 y;
        bool found = true;
        if (a1z) {
            if (ok1) { y.c0 = s; for (int k = 0; k < NL; k++) y.c1.l[k] = 0; }
            else if (c_sq) { for (int k = 0; k < NL; k++) y.c0.l[k] = 0; y.c1 = c; }   // c = (-a0)^((p+1)/4)
            else found = false;
        } else if (!ok1) {
            found = false;
        } else {
            Fp28 h;
            f_mul(h, a.c1, e);
            f_mul(h, h, half);                       // a1 e / 2
            if (c_sq) { y.c0 = c; y.c1 = h; }
            else { f_neg(y.c0, h); y.c1 = c; }
        }
        if (!found) {
            st = 3;
        } else {
            zkp28::fp28_to_wire(y0, y.c0);
            zkp28::fp28_to_wire(y1, y.c1);
            const bool big = w_is_zero(y1) ? w_gt_half(y0) : w_gt_half(y1);
            if (big != ((flags & 0x20) != 0)) { w_neg(y0); w_neg(y1); }
        }
    }
    const bool zero = st || inf;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        out[24 * i + k] = zero ? 0 : x0[k];
        out[24 * i + 6 + k] = zero ? 0 : x1[k];
        out[24 * i + 12 + k] = zero ? 0 : y0[k];
        out[24 * i + 18 + k] = zero ? 0 : y1[k];
    }
    if (inf && !st) out[24 * i + 12] = 1;  // identity (0, 1)
    out_inf[i] = inf && !st;
    status[i] = st;
}

// wire point -> compressed bytes: x with 0x80 | 0x20 (y is the larger of y and -y), or 0xc0 and zeros for the identity
template <bool ALIGNED>
__global__ void __launch_bounds__(TPB_C) k_g1_compress(const uint64_t* pts, const uint8_t* inf, size_t n, uint8_t* out) {
    const size_t i = (size_t)blockIdx.x * TPB_C + threadIdx.x;
    if (i >= n) return;
    uint8_t* dst = out + 48 * i;
    uint64_t x[6], y[6];
    const bool is_inf = inf && inf[i];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        x[k] = is_inf ? 0 : pts[12 * i + k];
        y[k] = pts[12 * i + 6 + k];
    }
    const uint64_t flags = is_inf ? (F_COMPRESSED | F_INFINITY) : (F_COMPRESSED | (w_gt_half(y) ? F_SORT : 0));
    x[5] &= FLAG_MASK;
    write_fe<ALIGNED>(dst, x, flags);
}
template <bool ALIGNED>
__global__ void __launch_bounds__(TPB_C) k_g2_compress(const uint64_t* pts, const uint8_t* inf, size_t n, uint8_t* out) {
    const size_t i = (size_t)blockIdx.x * TPB_C + threadIdx.x;
    if (i >= n) return;
    uint8_t* dst = out + 96 * i;
    uint64_t x0[6], x1[6], y0[6], y1[6];
    const bool is_inf = inf && inf[i];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        x0[k] = is_inf ? 0 : pts[24 * i + k];
        x1[k] = is_inf ? 0 : pts[24 * i + 6 + k];
        y0[k] = pts[24 * i + 12 + k];
        y1[k] = pts[24 * i + 18 + k];
    }
    const bool big = w_is_zero(y1) ? w_gt_half(y0) : w_gt_half(y1);
    const uint64_t flags = is_inf ? (F_COMPRESSED | F_INFINITY) : (F_COMPRESSED | (big ? F_SORT : 0));
    x1[5] &= FLAG_MASK;
    write_fe<ALIGNED>(dst, x1, flags);
    write_fe<ALIGNED>(dst + 48, x0, 0);
}

inline unsigned grid_c(size_t n) { return (unsigned)((n + TPB_C - 1) / TPB_C); }

}  // namespace

namespace zkp_cmp {

hipError_t decompress(int which, const void* bytes, size_t n, void* out, void* out_inf, void* status, hipStream_t s) {
    if (!n) return hipSuccess;
    const bool aligned = ((uintptr_t)bytes & 7u) == 0;
    const uint8_t* b = (const uint8_t*)bytes;
    uint64_t* o = (uint64_t*)out;
    uint8_t *oi = (uint8_t*)out_inf, *st = (uint8_t*)status;
    if (which == 1) {
        if (aligned) hipLaunchKernelGGL(k_g1_decompress<true>, dim3(grid_c(n)), dim3(TPB_C), 0, s, b, n, o, oi, st);
        else hipLaunchKernelGGL(k_g1_decompress<false>, dim3(grid_c(n)), dim3(TPB_C), 0, s, b, n, o, oi, st);
    } else {
        if (aligned) hipLaunchKernelGGL(k_g2_decompress<true>, dim3(grid_c(n)), dim3(TPB_C), 0, s, b, n, o, oi, st);
        else hipLaunchKernelGGL(k_g2_decompress<false>, dim3(grid_c(n)), dim3(TPB_C), 0, s, b, n, o, oi, st);
    }
    return hipGetLastError();
}

hipError_t compress(int which, const void* pts, const void* inf, size_t n, void* out_bytes, hipStream_t s) {
    if (!n) return hipSuccess;
    const bool aligned = ((uintptr_t)out_bytes & 7u) == 0;
    const uint64_t* p = (const uint64_t*)pts;
    const uint8_t* in = (const uint8_t*)inf;
    uint8_t* o = (uint8_t*)out_bytes;
    if (which == 1) {
        if (aligned) hipLaunchKernelGGL(k_g1_compress<true>, dim3(grid_c(n)), dim3(TPB_C), 0, s, p, in, n, o);
        else hipLaunchKernelGGL(k_g1_compress<false>, dim3(grid_c(n)), dim3(TPB_C), 0, s, p, in, n, o);
    } else {
        if (aligned) hipLaunchKernelGGL(k_g2_compress<true>, dim3(grid_c(n)), dim3(TPB_C), 0, s, p, in, n, o);
        else hipLaunchKernelGGL(k_g2_compress<false>, dim3(grid_c(n)), dim3(TPB_C), 0, s, p, in, n, o);
    }
    return hipGetLastError();
}

hipError_t sqrt_ref(int which, const uint64_t* a, size_t n, uint64_t* out, uint8_t* is_square, hipStream_t s) {
    if (!n) return hipSuccess;
    if (which == 1) hipLaunchKernelGGL(k_fp_sqrt, dim3(grid_c(n)), dim3(TPB_C), 0, s, a, n, out, is_square);
    else hipLaunchKernelGGL(k_fp2_sqrt, dim3(grid_c(n)), dim3(TPB_C), 0, s, a, n, out, is_square);
    return hipGetLastError();
}

}  // namespace zkp_cmp
