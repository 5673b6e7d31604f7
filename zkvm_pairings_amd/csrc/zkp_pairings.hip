// zkp_pairings.hip -- libzkp_pairings.so: C ABI (include/zkp_pairings.h) + the one-element-per-lane
// kernel family for gfx950.  The lane-cooperative hot-path kernels live in zkp_coop.hip and are
// dispatched from here when the context's kernel kind selects them.
//
// There is no CPU fallback anywhere in this file: every entry point either runs HIP kernels or
// returns a negative status.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include <new>
#include <string>

#include "../../include/zkp_pairings.h"
#include "../../include/zkp_poly.h"
#include "../../include/zkp_prove.h"
#include "../../include/zkp_fk20.h"
#include "../../include/zkp_cells.h"
#include "../../include/zkp_recover.h"
#include "../../include/zkp_bls.h"
#include "../../include/zkp_bls_agg.h"
#include "../../include/zkp_bls_grouped.h"
#include "../../include/zkp_bls_minsig.h"
#include "../../include/zkp_bls_agg_g2.h"
#include "zkp_field.hpp"
#include "zkp_coop.hpp"
#include "zkp_compress.hpp"
#include "zkp_msm.hpp"
#include "zkp_msm_plan.hpp"
#include "zkp_rlc.hpp"
#include "zkp_rlc_plan.hpp"
#include "zkp_groth16.hpp"
#include "zkp_groth16_plan.hpp"
#include "zkp_kzg.hpp"
#include "zkp_kzg_plan.hpp"
#include "zkp_poly.hpp"
#include "zkp_poly_plan.hpp"
#include "zkp_prove.hpp"
#include "zkp_prove_plan.hpp"
#include "zkp_fk20.hpp"
#include "zkp_cells.hpp"
#include "zkp_recover.hpp"
#include "zkp_bls.hpp"
#include "zkp_bls_agg.hpp"
#include "zkp_bls_grouped.hpp"
#include "zkp_bls_minsig.hpp"
#include "zkp_bls_agg_g2.hpp"
#include "zkp_fk20_plan.hpp"
#include "zkp_plan.hpp"

using namespace zkp;

// =============================================================================== kernels (thread family)
namespace {

constexpr int TPB = 64;   // threads per block for the scratch-heavy tower kernels
constexpr int KMAX = 4;   // pairs per shared-squaring Miller loop; larger k is split and multiplied

__device__ inline bool pair_live(const uint8_t* inf1, const uint8_t* inf2, size_t i) {
    return !((inf1 && inf1[i]) || (inf2 && inf2[i]));
}

// Miller loop over pairs [base, base+k) (k <= KMAX) with shared squarings; result NOT conjugated.
__device__ __attribute__((noinline)) void miller_group(Fp12* f, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1,
                                                        const uint8_t* inf2, size_t base, int k) {
    G1A ps[KMAX];
    G2A qs[KMAX];
    G2P rs[KMAX];
    bool live[KMAX];
    for (int j = 0; j < k; j++) {
        live[j] = pair_live(inf1, inf2, base + j);
        fp_load(&ps[j].x, g1 + 12 * (base + j));
        fp_load(&ps[j].y, g1 + 12 * (base + j) + 6);
        fp2_load(&qs[j].x, g2 + 24 * (base + j));
        fp2_load(&qs[j].y, g2 + 24 * (base + j) + 12);
        rs[j].x = qs[j].x;
        rs[j].y = qs[j].y;
        fp2_one(&rs[j].z);
    }
    fp12_one(f);
    Line l;
    bool found_one = false;
    for (int b = 63; b >= 0; b--) {
        bool bit = ((ZKP_BLS_X >> 1) >> b) & 1;
        if (!found_one) { found_one = bit; continue; }
        for (int j = 0; j < k; j++)
            if (live[j]) { doubling_step(&l, &rs[j]); ell(f, &l, &ps[j]); }
        if (bit)
            for (int j = 0; j < k; j++)
                if (live[j]) { addition_step(&l, &rs[j], &qs[j]); ell(f, &l, &ps[j]); }
        fp12_sqr(f, f);
    }
    for (int j = 0; j < k; j++)
        if (live[j]) { doubling_step(&l, &rs[j]); ell(f, &l, &ps[j]); }
}

// multi_miller_loop of one check of k pairs (any k): product of <=KMAX-pair groups, then conjugate
__device__ __attribute__((noinline)) void miller_check(Fp12* f, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1,
                                                        const uint8_t* inf2, size_t base, size_t k) {
    fp12_one(f);
    bool first = true;
    for (size_t off = 0; off < k; off += KMAX) {
        int kk = (int)((k - off) < (size_t)KMAX ? (k - off) : (size_t)KMAX);
        if (first) { miller_group(f, g1, g2, inf1, inf2, base + off, kk); first = false; }
        else { Fp12 g; miller_group(&g, g1, g2, inf1, inf2, base + off, kk); fp12_mul(f, f, &g); }
    }
    fp12_conj(f, f);  // x < 0
}

__global__ void __launch_bounds__(TPB) k_miller(const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2,
                                                 size_t n_checks, size_t k, uint64_t* out) {
    size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_checks) return;
    Fp12 f;
    miller_check(&f, g1, g2, inf1, inf2, i * k, k);
    fp12_store(out + 72 * i, &f);
}

__global__ void __launch_bounds__(TPB) k_final_exp(const uint64_t* in, size_t n, uint64_t* out) {
    size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    Fp12 f, r;
    fp12_load(&f, in + 72 * i);
    final_exponentiation(&r, &f);
    fp12_store(out + 72 * i, &r);
}

// fused: out[i] = final_exp(multi_miller_loop(check i)); optional ok byte + AND flag
__global__ void __launch_bounds__(TPB) k_pairing(const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2,
                                                  size_t n_checks, size_t k, uint64_t* out_gt, uint8_t* ok, int* all_ok) {
    size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_checks) return;
    Fp12 f, r;
    miller_check(&f, g1, g2, inf1, inf2, i * k, k);
    final_exponentiation(&r, &f);
    if (out_gt) fp12_store(out_gt + 72 * i, &r);
    if (ok || all_ok) {
        Fp12 one;
        fp12_one(&one);
        bool is_one = fp12_eq(&r, &one);
        if (ok) ok[i] = is_one ? 1 : 0;
        if (all_ok && !is_one) atomicAnd(all_ok, 0);
    }
}

__global__ void k_set_int(int* p, int v) { *p = v; }

// one wavefront that watches the shader clock counter (s_memtime) against the constant-rate wall clock (s_memrealtime)
// for about spin_us microseconds: out[0] = shader clock ticks, out[1] = wall clock ticks.  Launched beside a running
// pass it reports the clock the chip sustains under that load (bench.py: roofline.frac_at_sustained_clock).
__global__ void k_clock_probe(unsigned long long* out, unsigned long long wall_ticks) {
    if (threadIdx.x) return;
    const unsigned long long w0 = wall_clock64(), c0 = clock64();
    unsigned long long w1 = w0;
    while (w1 - w0 < wall_ticks) {
        __builtin_amdgcn_s_sleep(32);
        w1 = wall_clock64();
    }
    out[0] = clock64() - c0;
    out[1] = w1 - w0;
}

// one level of the Fp12 product tree, in place on wire records: buf[c] <- buf[c] * buf[c + h], c < m
__global__ void __launch_bounds__(TPB) k_fp12_mul_pairs(uint64_t* buf, size_t m, size_t h) {
    size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    Fp12 a, b;
    fp12_load(&a, buf + 72 * i);
    fp12_load(&b, buf + 72 * (i + h));
    fp12_mul(&a, &a, &b);
    fp12_store(buf + 72 * i, &a);
}

// *is_one = (gt == Gt::identity()) on a canonical wire record
__global__ void k_gt_is_one(const uint64_t* gt, int* is_one) {
    if (threadIdx.x || blockIdx.x) return;
    uint64_t d = gt[0] ^ 1ull;
    for (int i = 1; i < 72; i++) d |= gt[i];
    *is_one = d == 0 ? 1 : 0;
}

// reference src/g1.rs:49-62: 0 ok / 1 not on curve / 2 not torsion free
__global__ void __launch_bounds__(TPB) k_g1_valid(const uint64_t* g1, const uint8_t* inf, size_t n, uint8_t* status) {
    size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    if (inf && inf[i]) { status[i] = 0; return; }
    Fp x, y, t, u, b;
    fp_load(&x, g1 + 12 * i);
    fp_load(&y, g1 + 12 * i + 6);
    fp_sqr(&t, &y);
    fp_sqr(&u, &x);
    fp_mul(&u, &u, &x);
    fp_set(&b, K_M_B);
    fp_add(&u, &u, &b);
    if (!fp_eq(&t, &u)) { status[i] = 1; return; }
    // -[X][X]P == (beta x, y)  <=>  [X][X]P == (beta x, -y)
    uint64_t kx = ZKP_BLS_X;
    Jac<FpOps> q;
    jac_mul<FpOps>(&q, &x, &y, &kx, 1);
    Fp ax, ay;
    bool fin = jac_to_affine<FpOps>(&ax, &ay, &q);
    bool ok = false;
    if (fin) {
        jac_mul<FpOps>(&q, &ax, &ay, &kx, 1);
        Fp bx, ny, beta;
        fp_set(&beta, K_M_BETA);
        fp_mul(&bx, &x, &beta);
        fp_neg(&ny, &y);
        ok = jac_eq_affine<FpOps>(&q, &bx, &ny);
    }
    status[i] = ok ? 0 : 2;
}

// reference src/g2.rs:57-69: psi(P) == -[X]P
__global__ void __launch_bounds__(TPB) k_g2_valid(const uint64_t* g2, const uint8_t* inf, size_t n, uint8_t* status) {
    size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    if (inf && inf[i]) { status[i] = 0; return; }
    Fp2 x, y, t, u, b;
    fp2_load(&x, g2 + 24 * i);
    fp2_load(&y, g2 + 24 * i + 12);
    fp2_sqr(&t, &y);
    fp2_sqr(&u, &x);
    fp2_mul(&u, &u, &x);
    fp_set(&b.c0, K_M_B);
    fp_set(&b.c1, K_M_B);
    fp2_add(&u, &u, &b);
    if (!fp2_eq(&t, &u)) { status[i] = 1; return; }
    uint64_t kx = ZKP_BLS_X;
    Jac<Fp2Ops> q;
    jac_mul<Fp2Ops>(&q, &x, &y, &kx, 1);
    // psi(P) = (conj(x) * PSI_X, conj(y) * PSI_Y); compare with -[X]P
    Fp2 px, py, k;
    fp2_conj(&px, &x);
    fp2_const(&k, K_M_PSI_X_0, K_M_PSI_X_1);
    fp2_mul(&px, &px, &k);
    fp2_conj(&py, &y);
    fp2_const(&k, K_M_PSI_Y_0, K_M_PSI_Y_1);
    fp2_mul(&py, &py, &k);
    fp2_neg(&py, &py);
    status[i] = jac_eq_affine<Fp2Ops>(&q, &px, &py) ? 0 : 2;
}

__global__ void __launch_bounds__(TPB) k_g1_mul(const uint64_t* base, size_t stride, const uint64_t* sc, size_t n, uint64_t* out, uint8_t* out_inf) {
    size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    Fp x, y;
    fp_load(&x, base + stride * i);
    fp_load(&y, base + stride * i + 6);
    uint64_t k[4] = {sc[4 * i], sc[4 * i + 1], sc[4 * i + 2], sc[4 * i + 3]};
    Jac<FpOps> q;
    jac_mul<FpOps>(&q, &x, &y, k, 4);
    Fp ax, ay;
    bool fin = jac_to_affine<FpOps>(&ax, &ay, &q);
    fp_store(out + 12 * i, &ax);
    fp_store(out + 12 * i + 6, &ay);
    if (out_inf) out_inf[i] = fin ? 0 : 1;
}
__global__ void __launch_bounds__(TPB) k_g2_mul(const uint64_t* base, size_t stride, const uint64_t* sc, size_t n, uint64_t* out, uint8_t* out_inf) {
    size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    Fp2 x, y;
    fp2_load(&x, base + stride * i);
    fp2_load(&y, base + stride * i + 12);
    uint64_t k[4] = {sc[4 * i], sc[4 * i + 1], sc[4 * i + 2], sc[4 * i + 3]};
    Jac<Fp2Ops> q;
    jac_mul<Fp2Ops>(&q, &x, &y, k, 4);
    Fp2 ax, ay;
    bool fin = jac_to_affine<Fp2Ops>(&ax, &ay, &q);
    fp2_store(out + 24 * i, &ax);
    fp2_store(out + 24 * i + 12, &ay);
    if (out_inf) out_inf[i] = fin ? 0 : 1;
}

// batched field operation on canonical operands: 0 mul, 1 add (the zkVM precompile's two ops, src/fp.rs:376,443),
// 2 sub, 3 neg, 4 square, 5 invert (0 gives 0; the reference returns None, src/fp.rs:307-319)
__global__ void k_fp_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp x, y, r;
    fp_load(&x, a + 6 * i);
    if (op <= 2) fp_load(&y, b + 6 * i);
    switch (op) {
        case 0: fp_mul(&r, &x, &y); break;
        case 1: fp_add(&r, &x, &y); break;
        case 2: fp_sub(&r, &x, &y); break;
        case 3: fp_neg(&r, &x); break;
        case 4: fp_sqr(&r, &x); break;
        default: if (!fp_inv(&r, &x)) fp_zero(&r); break;
    }
    fp_store(out + 6 * i, &r);
}

// one tower operation per 72-u64 record (zkp_tower_op_batch, thread family): smaller tower elements occupy the leading
// coefficients of a record, the rest of the result is zero
__global__ void __launch_bounds__(TPB) k_tower_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint32_t repeat, uint64_t* out) {
    size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    Fp12 x, y, r;
    fp12_load(&x, a + 72 * i);
    if (b) fp12_load(&y, b + 72 * i);
    fp6_zero(&r.c0);
    fp6_zero(&r.c1);
    switch (op) {
        case ZKP_TOWER_FP2_MUL: fp2_mul(&r.c0.c0, &x.c0.c0, &y.c0.c0); break;
        case ZKP_TOWER_FP2_SQUARE: fp2_sqr(&r.c0.c0, &x.c0.c0); break;
        case ZKP_TOWER_FP6_MUL: fp6_mul(&r.c0, &x.c0, &y.c0); break;
        case ZKP_TOWER_FP6_SQUARE: fp6_sqr(&r.c0, &x.c0); break;
        case ZKP_TOWER_FP6_FROBENIUS: fp6_frob(&r.c0, &x.c0); break;
        case ZKP_TOWER_FP12_MUL: fp12_mul(&r, &x, &y); break;
        case ZKP_TOWER_FP12_SQUARE: fp12_sqr(&r, &x); break;
        case ZKP_TOWER_FP12_MUL_BY_014: fp12_mul_by_014(&r, &x, &y.c0.c0, &y.c0.c1, &y.c0.c2); break;
        case ZKP_TOWER_FP12_FROBENIUS: fp12_frob(&r, &x); break;
        case ZKP_TOWER_FP12_CONJUGATE: fp12_conj(&r, &x); break;
        case ZKP_TOWER_FP12_CYCLOTOMIC_SQUARE: fp12_cyclotomic_square(&r, &x); break;
        // a non-invertible input leaves the zero record (the reference returns None)
        case ZKP_TOWER_FP2_INVERT: if (!fp2_inv(&r.c0.c0, &x.c0.c0)) fp2_zero(&r.c0.c0); break;
        case ZKP_TOWER_FP2_MUL_BY_NONRESIDUE: fp2_mul_nr(&r.c0.c0, &x.c0.c0); break;
        case ZKP_TOWER_FP2_MUL_FP: fp2_mul_fp(&r.c0.c0, &x.c0.c0, &y.c0.c0.c0); break;
        case ZKP_TOWER_FP6_MUL_BY_1: fp6_mul_by_1(&r.c0, &x.c0, &y.c0.c0); break;
        case ZKP_TOWER_FP6_MUL_BY_01: fp6_mul_by_01(&r.c0, &x.c0, &y.c0.c0, &y.c0.c1); break;
        case ZKP_TOWER_FP6_MUL_BY_NONRESIDUE: fp6_mul_nr(&r.c0, &x.c0); break;
        case ZKP_TOWER_FP6_INVERT: if (!fp6_inv(&r.c0, &x.c0)) fp6_zero(&r.c0); break;
        case ZKP_TOWER_FP12_INVERT: if (!fp12_inv(&r, &x)) { fp6_zero(&r.c0); fp6_zero(&r.c1); } break;
        default:
            r = x;
            for (uint32_t k = 0; k < repeat; k++) { Fp12 t; fp12_cyclotomic_square(&t, &r); r = t; }
            break;
    }
    fp12_store(out + 72 * i, &r);
}

// ---- uncompressed byte codec: nfp big-endian 48-byte field elements per point (2 for G1, 4 for G2).
// G2 stores c1 before c0, so element e of the byte string is wire element (e ^ 1) when nfp == 4.
// ALIGNED: the byte strings start on an 8-byte boundary (96 and 192 are multiples of 8): a big-endian word is one 64-bit load + a
// byte swap instead of eight byte loads.
template <bool ALIGNED>
__device__ __forceinline__ uint64_t be64_load(const uint8_t* p) {
    if (ALIGNED) return __builtin_bswap64(*reinterpret_cast<const uint64_t*>(p));
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) v = (v << 8) | p[b];
    return v;
}
template <bool ALIGNED>
__global__ void k_decode(const uint8_t* bytes, size_t n, int nfp, uint64_t* out, uint8_t* out_inf, uint8_t* status) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* src = bytes + i * 48 * nfp;
    const uint8_t flags = src[0] & 0xe0;
    uint8_t st = 0, inf = 0;
    if (flags & 0xa0) st = 2;                       // compressed or sort flag: not an uncompressed point
    if (!st && (flags & 0x40)) {
        inf = 1;
        uint64_t any = be64_load<ALIGNED>(src) & 0x1fffffffffffffffULL;
        for (int w = 1; w < 6 * nfp; w++) any |= be64_load<ALIGNED>(src + 8 * w);
        if (any) st = 2;
    }
    for (int e = 0; e < nfp; e++) {
        uint64_t limbs[6];
        for (int w = 0; w < 6; w++) {
            uint64_t v = be64_load<ALIGNED>(src + 48 * e + 8 * w);
            if (e == 0 && w == 0) v &= 0x1fffffffffffffffULL;   // strip the flag bits
            limbs[5 - w] = v;
        }
        if (!st && !inf && !fp_wire_is_canonical(limbs)) st = 1;
        const int we = nfp == 4 ? (e ^ 1) : e;
        for (int w = 0; w < 6; w++) out[(i * nfp + we) * 6 + w] = (st || inf) ? 0 : limbs[w];
    }
    if (inf && !st) out[(i * nfp + nfp / 2) * 6] = 1;   // identity is (0, 1) like the reference (src/g1.rs:25-31)
    out_inf[i] = inf && !st;
    status[i] = st;
}
template <bool ALIGNED>
__global__ void k_encode(const uint64_t* pts, const uint8_t* inf, size_t n, int nfp, uint8_t* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t* dst = out + i * 48 * nfp;
    const bool is_inf = inf && inf[i];
    for (int e = 0; e < nfp; e++) {
        const int we = nfp == 4 ? (e ^ 1) : e;
        for (int w = 0; w < 6; w++) {
            uint64_t v = is_inf ? 0 : pts[(i * nfp + we) * 6 + (5 - w)];
            if (is_inf && e == 0 && w == 0) v = 0x4000000000000000ULL;
            if (ALIGNED) {
                *reinterpret_cast<uint64_t*>(dst + 48 * e + 8 * w) = __builtin_bswap64(v);
            } else {
                for (int b = 0; b < 8; b++) dst[48 * e + 8 * w + b] = (uint8_t)(v >> (56 - 8 * b));
            }
        }
    }
}

// zkp_points_check_batch: one status byte per point from the decode status (0 ok, 1 coordinate >= p, 2 malformed) and the is_valid
// status (0, 1 not on the curve, 2 not torsion free): 0 valid (or a well-formed infinity), 1, 2 as decoded, 3 not on the curve, 4 not
// in the subgroup (zkp_point_status).  A point that is not valid is flagged as infinity for the Miller loop (it contributes the
// neutral line: no arithmetic on garbage) - its check is failed by k_checks_merge whatever the pairing product says.
__global__ void k_points_merge(const uint8_t* dec, const uint8_t* val, uint8_t* inf, size_t n, uint8_t* st_out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t st = dec[i] ? dec[i] : (val[i] ? (uint8_t)(val[i] + 2) : (uint8_t)0);
    st_out[i] = st;
    if (st) inf[i] = 1;
}
__global__ void k_checks_merge(const uint8_t* st1, const uint8_t* st2, size_t n_checks, size_t k, uint8_t* ok, int* all_ok) {
    size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_checks) return;
    uint8_t bad = 0;
    for (size_t j = 0; j < k; j++) bad |= st1[c * k + j] | st2[c * k + j];
    if (bad) {
        if (ok) ok[c] = 0;
        if (all_ok) atomicAnd(all_ok, 0);
    }
}

// ---- round 5: no pairing work on checks already known to fail.  k_checks_compact lists the checks whose 2k points are all valid
// (idx[0 .. *count), any order) and zeroes the ok byte of the others; k_gather_checks copies the listed checks' points next to each
// other; k_scatter_ok puts the compact ok bytes back.  (wave-aggregated: one atomicAdd per wavefront)
__global__ void k_checks_compact(const uint8_t* st1, const uint8_t* st2, size_t n_checks, size_t k, uint32_t* idx, uint32_t* count, uint8_t* ok) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool good = false;
    if (c < n_checks) {
        uint8_t bad = 0;
        for (size_t j = 0; j < k; j++) bad |= st1[c * k + j] | st2[c * k + j];
        good = !bad;
        if (bad && ok) ok[c] = 0;
    }
    const unsigned long long m = __ballot(good);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == __ffsll((long long)m) - 1) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1);
    if (good) idx[base + __popcll(m & ((1ull << lane) - 1))] = (uint32_t)c;
}
// out[j * words + w] = in[idx[j] * words + w]: `words` 64-bit words (or bytes: T = uint8_t) per check.  Round 6: the number of listed
// checks is read from DEVICE memory (*count <= n_max; the grid covers n_max checks) - the host never learns it
template <class T>
__global__ void k_gather_checks(const T* in, const uint32_t* idx, const uint32_t* count, size_t n_max, size_t words, T* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t m = *count < n_max ? *count : n_max;
    if (i >= m * words) return;
    const size_t j = i / words, w = i - j * words;
    out[i] = in[(size_t)idx[j] * words + w];
}
__global__ void k_scatter_ok(const uint8_t* okc, const uint32_t* idx, const uint32_t* count, size_t n_max, uint8_t* ok) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t m = *count < n_max ? *count : n_max;
    if (j < m) ok[idx[j]] = okc[j];
}
// the AND over all checks is 0 as soon as one check failed its validity tests, whatever the pairings of the others say
__global__ void k_flag_if_fewer(int* all_ok, const uint32_t* count, uint32_t n_checks) {
    if (*count < n_checks) *all_ok = 0;
}

// every 6-limb element of a wire buffer must be < p
__global__ void k_check_canonical(const uint64_t* a, size_t n_fp, int* bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_fp) return;
    if (!fp_wire_is_canonical(a + 6 * i)) atomicOr(bad, 1);
}

}  // namespace

// =============================================================================== context
struct zkp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int validate = 0;
    int kernel = ZKP_KERNEL_AUTO;
    std::string err;
    // grow-only device workspace for the host-pointer API
    void* buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int* d_flag = nullptr;      // [0] product check result, [1] AND flag of the host entry points, [2] sticky validation word of the *_dev calls
    hipEvent_t ws_busy = nullptr;   // recorded at the end of every *_dev call: the next call (on whatever stream) waits for it
    void* msm_ws = nullptr;     // grow-only workspace of the MSM calls (zkp_msm_plan.hpp layout)
    size_t msm_cap = 0;
    void* rlc_ws = nullptr;     // grow-only workspace of the RLC batch check (zkp_rlc_plan.hpp layout)
    size_t rlc_cap = 0;
    void* g16_ws = nullptr;     // grow-only workspace of the Fr fold and the Groth16 verifier (zkp_groth16_plan.hpp layout)
    size_t g16_cap = 0;
    void* kzg_ws = nullptr;     // grow-only workspace of the batched inversion, the evaluation and the KZG verifier (zkp_kzg_plan.hpp layouts)
    size_t kzg_cap = 0;
    uint32_t* kzg_dom = nullptr;   // omega^i for i < 2^kzg_dom_log2, Montgomery form: the evaluation's domain table (-1: none yet)
    int kzg_dom_log2 = -1;
    uint32_t* poly_coset = nullptr;   // the NTT's coset tables (zkp_poly_plan.hpp: COSET_BYTES), built at the first coset call
    void* prove_ws = nullptr;   // grow-only workspace of the QAP quotient and the Groth16 prover (zkp_prove_plan.hpp layout)
    size_t prove_cap = 0;
    void* fk20_ws = nullptr;    // grow-only workspace of the G1 NTT and of FK20 (zkp_fk20_plan.hpp: Jacobian records, FK20's field elements)
    size_t fk20_cap = 0;
    uint64_t* g1ntt_split = nullptr;   // the split twiddles of kzg_dom, entry for entry (-1: none yet): rebuilt when that table grows
    int g1ntt_split_log2 = -1;
    void* bls_ws = nullptr;     // grow-only workspace of hash-to-G2 and the BLS verifier (zkp_bls_plan.hpp layout)
    size_t bls_cap = 0;
    void* agg_ws = nullptr;     // grow-only workspace of the G1 segment sums and FastAggregateVerify (zkp_bls_agg_plan.hpp layout)
    size_t agg_cap = 0;
    void* grp_ws = nullptr;     // grow-only workspace of the scaled segment sums and the grouped verifiers (zkp_bls_grouped_plan.hpp layout)
    size_t grp_cap = 0;
    void* minsig_ws = nullptr;  // grow-only workspace of hash-to-G1 and the min-sig BLS verifiers (zkp_bls_minsig_plan.hpp layout)
    size_t minsig_cap = 0;
    uint64_t* prod = nullptr;   // Fp12 records of the product tree (zkp_fp12_product / zkp_miller_product)
    size_t prod_cap = 0;
    // host-pointer pairing entry points on large batches: slices of host_slice pairs, two workspace slots, copies of
    // the next / previous slice on their own streams while the current slice computes
    struct HostSlot {
        void* buf[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // g1 g2 inf1 inf2 gt ok
        size_t cap[6] = {0, 0, 0, 0, 0, 0};
        hipEvent_t in = nullptr, done = nullptr, out = nullptr;
    } hs[2];
    hipStream_t s_in = nullptr, s_out = nullptr;
    size_t host_slice = (size_t)1 << 19;
    hipDeviceProp_t prop;
    zkp::CoopState coop;
    // zkp_points_check_batch: decoded points, infinity flags, decode / is_valid / merged status bytes, ok bytes (grow-only)
    void* pc[18] = {};
    size_t pc_cap[18] = {};
    // one-rank-per-GPU communicator (zkp_comm_init_rank); null until then
    ncclComm_t comm = nullptr;
    int comm_nranks = 0, comm_rank = 0;
    // (nranks + 3) Fp12 records owned by the communicator: [0] this rank's record, [1..R] the gathered ones, [R+1] their product, [R+2] Gt.
    // Allocated by zkp_comm_init_rank, so that no allocation stands between a rank and the all-gather its peers wait in.
    uint64_t* comm_buf = nullptr;
};

namespace {

static const uint64_t GT_IDENTITY[72] = {1};

#define HIPCHK(ctx, call)                                                                       \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess) {                                                                \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                    \
            return e__ == hipErrorOutOfMemory ? ZKP_ERR_OOM : ZKP_ERR_HIP;                      \
        }                                                                                       \
    } while (0)

int ensure(zkp_ctx* c, int slot, size_t bytes) {
    if (bytes <= c->cap[slot]) return ZKP_OK;
    if (c->buf[slot]) { HIPCHK(c, hipFree(c->buf[slot])); c->buf[slot] = nullptr; c->cap[slot] = 0; }
    HIPCHK(c, hipMalloc(&c->buf[slot], bytes));
    zkp_dbg_alloc(slot == 0 ? "ctx.buf0" : slot == 1 ? "ctx.buf1" : slot == 4 ? "ctx.buf4" : "ctx.buf", c->buf[slot], bytes);
    c->cap[slot] = bytes;
    return ZKP_OK;
}

inline unsigned grid_for(size_t n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

// status of a call into the cooperative family: the HIP error (launch configuration, out of memory, ...) goes to zkp_last_error
int coop_rc(zkp_ctx* c, const char* what, hipError_t e) {
    if (e == hipSuccess) return ZKP_OK;
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? ZKP_ERR_OOM : ZKP_ERR_HIP;
}

int bind(zkp_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    return ZKP_OK;
}

// ---- device-pointer implementations (shared by both API flavours)
int miller_product_dev(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n, uint64_t* out,
                       hipStream_t s);
int miller_dev(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n_checks, size_t k,
               uint64_t* out, hipStream_t s) {
    if (n_checks == 0) return ZKP_OK;
    if (k >= 64 && n_checks <= 16) {
        // few checks with long term lists: spread each check's pairs over the GPU (eight per accumulator) and fold the
        // values with the product tree, instead of walking the check's groups one after the other
        for (size_t ck = 0; ck < n_checks; ck++) {
            int rc = miller_product_dev(c, g1 + 12 * ck * k, g2 + 24 * ck * k, i1 ? i1 + ck * k : nullptr, i2 ? i2 + ck * k : nullptr, k,
                                        out + 72 * ck, s);
            if (rc) return rc;
        }
        return ZKP_OK;
    }
    if (zkp::coop_selected(&c->coop, c->kernel) && zkp::coop_supports_k(k))
        return coop_rc(c, "coop_miller", zkp::coop_miller(&c->coop, g1, g2, i1, i2, n_checks, k, out, s));
    hipLaunchKernelGGL(k_miller, dim3(grid_for(n_checks, TPB)), dim3(TPB), 0, s, g1, g2, i1, i2, n_checks, k, out);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}
int final_exp_dev(zkp_ctx* c, const uint64_t* f, size_t n, uint64_t* out, hipStream_t s) {
    if (n == 0) return ZKP_OK;
    if (zkp::coop_selected(&c->coop, c->kernel))
        return coop_rc(c, "coop_final_exp", zkp::coop_final_exp(&c->coop, f, n, out, nullptr, nullptr, s));
    hipLaunchKernelGGL(k_final_exp, dim3(grid_for(n, TPB)), dim3(TPB), 0, s, f, n, out);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}
// n_dev (device pointer, cooperative family only): the number of checks that really exist (<= n_checks) - see zkp::coop_pairing
int pairing_dev(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n_checks, size_t k,
                uint64_t* out_gt, uint8_t* ok, int* all_ok, hipStream_t s, bool reset_flag = true, const uint32_t* n_dev = nullptr) {
    if (all_ok && reset_flag) {
        hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, s, all_ok, 1);
        HIPCHK(c, hipGetLastError());
    }
    if (n_checks == 0) return ZKP_OK;
    if (zkp::coop_selected(&c->coop, c->kernel) && zkp::coop_supports_k(k))
        return coop_rc(c, "coop_pairing", zkp::coop_pairing(&c->coop, g1, g2, i1, i2, n_checks, k, out_gt, ok, all_ok, s, n_dev));
    if (n_dev) { c->err = "pairing_dev: a device-resident count needs the cooperative kernel family"; return ZKP_ERR_ARG; }
    hipLaunchKernelGGL(k_pairing, dim3(grid_for(n_checks, TPB)), dim3(TPB), 0, s, g1, g2, i1, i2, n_checks, k, out_gt, ok, all_ok);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}

int ensure_prod(zkp_ctx* c, size_t records) {
    const size_t bytes = (records + 2) * 576;   // two spare records: product and Gt of zkp_pairing_product_check
    if (bytes <= c->prod_cap) return ZKP_OK;
    if (c->prod) { HIPCHK(c, hipFree(c->prod)); c->prod = nullptr; c->prod_cap = 0; }
    HIPCHK(c, hipMalloc((void**)&c->prod, bytes));
    zkp_dbg_alloc("ctx.prod", c->prod, bytes);
    c->prod_cap = bytes;
    return ZKP_OK;
}

// buf[0] <- prod_{i<n} buf[i] (n >= 1), destroying buf[1..n): ceil(log2 n) launches, level l multiplies element c
// by element c + ceil(n_l / 2)
int fp12_product_inplace(zkp_ctx* c, uint64_t* buf, size_t n, hipStream_t s) {
    const bool coop = zkp::coop_selected(&c->coop, c->kernel);
    while (n > 1) {
        const size_t h = (n + 1) / 2, m = n - h;
        if (coop) {
            if (int rc = coop_rc(c, "coop_fp12_mul_pairs", zkp::coop_fp12_mul_pairs(&c->coop, buf, m, h, s))) return rc;
        } else {
            hipLaunchKernelGGL(k_fp12_mul_pairs, dim3(grid_for(m, TPB)), dim3(TPB), 0, s, buf, m, h);
            HIPCHK(c, hipGetLastError());
        }
        n = h;
    }
    return ZKP_OK;
}

int fp12_product_dev(zkp_ctx* c, const uint64_t* f, size_t n, uint64_t* out, hipStream_t s) {
    if (n == 0) { HIPCHK(c, hipMemcpyAsync(out, GT_IDENTITY, 576, hipMemcpyHostToDevice, s)); return ZKP_OK; }
    int rc = ensure_prod(c, n);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->prod, f, n * 576, hipMemcpyDeviceToDevice, s));
    if ((rc = fp12_product_inplace(c, c->prod, n, s))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->prod, 576, hipMemcpyDeviceToDevice, s));
    return ZKP_OK;
}

// multi_miller_loop over the whole batch as ONE check: the pairs are taken eight at a time (one shared accumulator
// per eight pairs), the n/8 values are multiplied by the product tree.  Result left in c->prod[0..72) and copied to out.
int miller_product_dev(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n, uint64_t* out,
                       hipStream_t s) {
    if (n == 0) { HIPCHK(c, hipMemcpyAsync(out, GT_IDENTITY, 576, hipMemcpyHostToDevice, s)); return ZKP_OK; }
    constexpr size_t PG = 8;   // pairs per accumulator
    const size_t n4 = n / PG, r = n % PG, nv = n4 + (r ? 1 : 0);
    int rc = ensure_prod(c, nv);
    if (rc) return rc;
    if (n4 && (rc = miller_dev(c, g1, g2, i1, i2, n4, PG, c->prod, s))) return rc;
    if (r && (rc = miller_dev(c, g1 + 12 * PG * n4, g2 + 24 * PG * n4, i1 ? i1 + PG * n4 : nullptr, i2 ? i2 + PG * n4 : nullptr, 1, r,
                              c->prod + 72 * n4, s)))
        return rc;
    if ((rc = fp12_product_inplace(c, c->prod, nv, s))) return rc;
    if (out) HIPCHK(c, hipMemcpyAsync(out, c->prod, 576, hipMemcpyDeviceToDevice, s));
    return ZKP_OK;
}

// prod_i e(P_i, Q_i) == Gt::identity() with ONE final exponentiation; out_gt and is_one are device pointers, each optional
int product_check_dev(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n, uint64_t* out_gt,
                      int* is_one, hipStream_t s) {
    int rc = ensure_prod(c, n / 8 + 1);
    if (rc) return rc;
    if ((rc = miller_product_dev(c, g1, g2, i1, i2, n, n ? nullptr : c->prod, s))) return rc;
    const size_t nv = n / 8 + (n % 8 ? 1 : 0);
    uint64_t* gt = c->prod + 72 * (nv + 1);      // spare record (ensure_prod keeps two)
    if ((rc = final_exp_dev(c, c->prod, 1, gt, s))) return rc;
    if (out_gt) HIPCHK(c, hipMemcpyAsync(out_gt, gt, 576, hipMemcpyDeviceToDevice, s));
    if (is_one) {
        hipLaunchKernelGGL(k_gt_is_one, dim3(1), dim3(64), 0, s, gt, is_one);
        HIPCHK(c, hipGetLastError());
    }
    return ZKP_OK;
}

// canonical-range validation of a host-API input already copied to the device
int validate_dev(zkp_ctx* c, const uint64_t* d, size_t n_fp) {
    if (!c->validate || n_fp == 0) return ZKP_OK;
    HIPCHK(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_check_canonical, dim3(grid_for(n_fp, 256)), dim3(256), 0, c->stream, d, n_fp, c->d_flag);
    HIPCHK(c, hipGetLastError());
    int bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) { c->err = "input limbs >= p"; return ZKP_ERR_NONCANONICAL; }
    return ZKP_OK;
}

struct Staged { const uint64_t *g1, *g2; const uint8_t *i1, *i2; };

int ensure_slot(zkp_ctx* c, zkp_ctx::HostSlot* h, int which, size_t bytes) {
    if (bytes <= h->cap[which]) return ZKP_OK;
    if (h->buf[which]) { HIPCHK(c, hipFree(h->buf[which])); h->buf[which] = nullptr; h->cap[which] = 0; }
    HIPCHK(c, hipMalloc(&h->buf[which], bytes));
    zkp_dbg_alloc(which == 0 ? "slot.g1" : which == 1 ? "slot.g2" : which == 4 ? "slot.gt" : "slot.other", h->buf[which], bytes);
    h->cap[which] = bytes;
    return ZKP_OK;
}

// pairing()/pairing check of n_checks x k pairs from HOST arrays in slices: while slice i computes on the context's
// stream, the host thread uploads slice i+1 (copy-in stream) and downloads the results of slice i-1 (copy-out stream).
// out_gt / ok / all_ok are host pointers, each optional.
int host_sliced_impl(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n_checks, size_t k,
                     uint64_t* out_gt, uint8_t* ok, int* all_ok) {
    const zkp::plan::Slices sl = zkp::plan::plan_slices(c->host_slice, n_checks, k);
    const size_t sc = sl.checks_per_slice, nsl = sl.n_slices;
    int rc;
    if (!c->s_in) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            HIPCHK(c, hipEventCreateWithFlags(&c->hs[i].in, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->hs[i].done, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->hs[i].out, hipEventDisableTiming));
        }
    }
    for (int i = 0; i < 2; i++) {
        zkp_ctx::HostSlot* h = &c->hs[i];
        if ((rc = ensure_slot(c, h, 0, sc * k * 96)) || (rc = ensure_slot(c, h, 1, sc * k * 192))) return rc;
        if (inf1 && (rc = ensure_slot(c, h, 2, sc * k))) return rc;
        if (inf2 && (rc = ensure_slot(c, h, 3, sc * k))) return rc;
        if (out_gt && (rc = ensure_slot(c, h, 4, sc * 576))) return rc;
        if ((rc = ensure_slot(c, h, 5, sc))) return rc;
    }
    hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, c->stream, c->d_flag + 1, 1);
    HIPCHK(c, hipGetLastError());
    auto upload = [&](size_t i) -> int {
        zkp_ctx::HostSlot* h = &c->hs[i & 1];
        const size_t c0 = i * sc, ns = n_checks - c0 < sc ? n_checks - c0 : sc, p0 = c0 * k, np = ns * k;
        if (i >= 2) HIPCHK(c, hipStreamWaitEvent(c->s_in, h->done, 0));   // slice i-2 has finished reading these buffers
        HIPCHK(c, hipMemcpyAsync(h->buf[0], g1 + 12 * p0, np * 96, hipMemcpyHostToDevice, c->s_in));
        HIPCHK(c, hipMemcpyAsync(h->buf[1], g2 + 24 * p0, np * 192, hipMemcpyHostToDevice, c->s_in));
        if (inf1) HIPCHK(c, hipMemcpyAsync(h->buf[2], inf1 + p0, np, hipMemcpyHostToDevice, c->s_in));
        if (inf2) HIPCHK(c, hipMemcpyAsync(h->buf[3], inf2 + p0, np, hipMemcpyHostToDevice, c->s_in));
        HIPCHK(c, hipEventRecord(h->in, c->s_in));
        return ZKP_OK;
    };
    auto download = [&](size_t i) -> int {
        zkp_ctx::HostSlot* h = &c->hs[i & 1];
        const size_t c0 = i * sc, ns = n_checks - c0 < sc ? n_checks - c0 : sc;
        HIPCHK(c, hipStreamWaitEvent(c->s_out, h->done, 0));
        if (out_gt) HIPCHK(c, hipMemcpyAsync(out_gt + 72 * c0, h->buf[4], ns * 576, hipMemcpyDeviceToHost, c->s_out));
        if (ok) HIPCHK(c, hipMemcpyAsync(ok + c0, h->buf[5], ns, hipMemcpyDeviceToHost, c->s_out));
        HIPCHK(c, hipEventRecord(h->out, c->s_out));
        return ZKP_OK;
    };
    if ((rc = upload(0))) return rc;
    for (size_t i = 0; i < nsl; i++) {
        zkp_ctx::HostSlot* h = &c->hs[i & 1];
        const size_t c0 = i * sc, ns = n_checks - c0 < sc ? n_checks - c0 : sc;
        HIPCHK(c, hipStreamWaitEvent(c->stream, h->in, 0));
        if (i >= 2) HIPCHK(c, hipStreamWaitEvent(c->stream, h->out, 0));   // results of slice i-2 have left the output buffers
        if ((rc = pairing_dev(c, (const uint64_t*)h->buf[0], (const uint64_t*)h->buf[1], inf1 ? (const uint8_t*)h->buf[2] : nullptr,
                              inf2 ? (const uint8_t*)h->buf[3] : nullptr, ns, k, out_gt ? (uint64_t*)h->buf[4] : nullptr, (uint8_t*)h->buf[5],
                              c->d_flag + 1, c->stream, false)))
            return rc;
        HIPCHK(c, hipEventRecord(h->done, c->stream));
        if (i + 1 < nsl && (rc = upload(i + 1))) return rc;
        if (i >= 1 && (rc = download(i - 1))) return rc;
    }
    if ((rc = download(nsl - 1))) return rc;
    int flag = 1;
    HIPCHK(c, hipMemcpyAsync(&flag, c->d_flag + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->s_out));
    if (all_ok) *all_ok = flag;
    return ZKP_OK;
}

// an error must not leave copies from / into the caller's arrays in flight
int host_sliced(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n_checks, size_t k,
                uint64_t* out_gt, uint8_t* ok, int* all_ok) {
    const int rc = host_sliced_impl(c, g1, g2, inf1, inf2, n_checks, k, out_gt, ok, all_ok);
    if (rc != ZKP_OK) {
        if (c->s_in) (void)hipStreamSynchronize(c->s_in);
        (void)hipStreamSynchronize(c->stream);
        if (c->s_out) (void)hipStreamSynchronize(c->s_out);
    }
    return rc;
}

// Staging of a host-pointer call on the context's stream.  in() grows a workspace slot and queues the upload of a host array into it
// (a null host pointer gives a null device pointer and grows nothing); out() grows a slot and notes its download into a host array
// (none for a null one), which send() queues behind the work.  The first failure is kept (status()) and makes every later step a
// no-op, so one check before the launch covers them all.
struct Staging {
    zkp_ctx* c;
    int rc = ZKP_OK;
    struct Copy { void* host; const void* dev; size_t bytes; } down[8];   // the most a call needs: the prover's seven
    int n_down = 0;
    explicit Staging(zkp_ctx* ctx) : c(ctx) {}
    int status() const { return rc; }
    void* slot(int i, size_t bytes) {
        if (!rc) rc = ensure(c, i, bytes);
        return rc ? nullptr : c->buf[i];
    }
    const void* put(void* dev, const void* host, size_t bytes) {
        if (!rc && host && bytes) rc = coop_rc(c, "hipMemcpyAsync (upload)", hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
        return host ? dev : nullptr;
    }
    void get(void* host, const void* dev, size_t bytes) {
        if (!host || !bytes || rc) return;
        if (n_down == 8) { c->err = "Staging: more than eight downloads"; rc = ZKP_ERR_ARG; return; }
        down[n_down++] = {host, dev, bytes};
    }
    const void* in(int i, const void* host, size_t bytes) { return host ? put(slot(i, bytes), host, bytes) : nullptr; }
    void* out(int i, void* host, size_t bytes) {
        void* d = slot(i, bytes);
        get(host, d, bytes);
        return d;
    }
    int send() {
        for (int i = 0; i < n_down && !rc; i++)
            rc = coop_rc(c, "hipMemcpyAsync (download)", hipMemcpyAsync(down[i].host, down[i].dev, down[i].bytes, hipMemcpyDeviceToHost, c->stream));
        return rc;
    }
};

// Host-pointer entry points copy from / into the caller's arrays asynchronously: whatever way such a call returns
// (HIPCHK included), nothing may still be in flight - the context's stream is drained on the way out.
struct HostIO : Staging {
    bool bound;
    explicit HostIO(zkp_ctx* ctx) : Staging(ctx) {
        rc = bind(c);
        bound = rc == ZKP_OK;
        if (bound) (void)hipStreamWaitEvent(c->stream, c->ws_busy, 0);   // earlier *_dev calls may still be using the workspace on other streams
    }
    ~HostIO() {
        if (!bound) return;
        (void)hipEventRecord(c->ws_busy, c->stream);
        (void)hipStreamSynchronize(c->stream);
    }
    // the noted downloads, then one synchronisation
    int finish() {
        if (!send()) rc = coop_rc(c, "hipStreamSynchronize", hipStreamSynchronize(c->stream));
        return rc;
    }
};

// a (g1,g2,inf1,inf2) pair batch to workspace slots 0..3, range-checked in validation mode
int stage_pairs(Staging& io, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t np, Staged* st) {
    st->g1 = (const uint64_t*)io.in(0, g1, np * 96);
    st->g2 = (const uint64_t*)io.in(1, g2, np * 192);
    st->i1 = (const uint8_t*)io.in(2, inf1, np);
    st->i2 = (const uint8_t*)io.in(3, inf2, np);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(io.c, st->g1, np * 2)) || (rc = validate_dev(io.c, st->g2, np * 4))) return rc;
    return ZKP_OK;
}

}  // namespace

// =============================================================================== C ABI
extern "C" {

int zkp_abi_version(void) { return 4; }

const char* zkp_strerror(int status) {
    switch (status) {
        case ZKP_OK: return "ok";
        case ZKP_ERR_ARG: return "bad argument";
        case ZKP_ERR_NO_DEVICE: return "no usable HIP device";
        case ZKP_ERR_HIP: return "HIP runtime error";
        case ZKP_ERR_NONCANONICAL: return "non-canonical field element in input";
        case ZKP_ERR_OOM: return "out of device memory";
        case ZKP_ERR_COMM: return "RCCL error / no communicator";
        default: return "unknown status";
    }
}

const uint64_t* zkp_gt_identity(void) { return GT_IDENTITY; }

int zkp_init(int device, zkp_ctx** out_ctx) {
    if (!out_ctx) return ZKP_ERR_ARG;
    *out_ctx = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return ZKP_ERR_NO_DEVICE;
    zkp_ctx* c = new (std::nothrow) zkp_ctx();
    if (!c) return ZKP_ERR_OOM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&c->prop, device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess || hipEventCreateWithFlags(&c->ws_busy, hipEventDisableTiming) != hipSuccess ||
        hipMalloc((void**)&c->d_flag, 3 * sizeof(int)) != hipSuccess || hipMemset(c->d_flag, 0, 3 * sizeof(int)) != hipSuccess) {
        zkp_free(c);
        return ZKP_ERR_NO_DEVICE;
    }
    if (zkp::coop_init(&c->coop, c->prop) != hipSuccess) {
        zkp_free(c);
        return ZKP_ERR_HIP;
    }
    if (const char* hsl = getenv("ZKP_HOST_SLICE")) {
        c->host_slice = (size_t)atol(hsl);
        if (c->host_slice < 64) c->host_slice = 64;
    }
    const char* env = getenv("ZKP_KERNEL");
    if (env) {
        if (!strcmp(env, "thread")) c->kernel = ZKP_KERNEL_THREAD;
        else if (!strcmp(env, "coop")) c->kernel = ZKP_KERNEL_COOP;
    }
    *out_ctx = c;
    return ZKP_OK;
}

void zkp_free(zkp_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->comm) { (void)ncclCommDestroy(c->comm); c->comm = nullptr; }
    if (c->comm_buf) { (void)hipFree(c->comm_buf); c->comm_buf = nullptr; }
    zkp::coop_free(&c->coop);
    for (int i = 0; i < 8; i++)
        if (c->buf[i]) (void)hipFree(c->buf[i]);
    for (int i = 0; i < 18; i++)
        if (c->pc[i]) (void)hipFree(c->pc[i]);
    if (c->d_flag) (void)hipFree(c->d_flag);
    if (c->prod) (void)hipFree(c->prod);
    if (c->msm_ws) (void)hipFree(c->msm_ws);
    if (c->rlc_ws) (void)hipFree(c->rlc_ws);
    if (c->g16_ws) (void)hipFree(c->g16_ws);
    if (c->kzg_ws) (void)hipFree(c->kzg_ws);
    if (c->prove_ws) (void)hipFree(c->prove_ws);
    if (c->kzg_dom) (void)hipFree(c->kzg_dom);
    if (c->poly_coset) (void)hipFree(c->poly_coset);
    if (c->fk20_ws) (void)hipFree(c->fk20_ws);
    if (c->bls_ws) (void)hipFree(c->bls_ws);
    if (c->agg_ws) (void)hipFree(c->agg_ws);
    if (c->grp_ws) (void)hipFree(c->grp_ws);
    if (c->minsig_ws) (void)hipFree(c->minsig_ws);
    if (c->g1ntt_split) (void)hipFree(c->g1ntt_split);
    for (int i = 0; i < 2; i++) {
        for (int j = 0; j < 6; j++)
            if (c->hs[i].buf[j]) (void)hipFree(c->hs[i].buf[j]);
        if (c->hs[i].in) (void)hipEventDestroy(c->hs[i].in);
        if (c->hs[i].done) (void)hipEventDestroy(c->hs[i].done);
        if (c->hs[i].out) (void)hipEventDestroy(c->hs[i].out);
    }
    if (c->s_in) (void)hipStreamDestroy(c->s_in);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ws_busy) (void)hipEventDestroy(c->ws_busy);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* zkp_last_error(const zkp_ctx* c) { return c ? c->err.c_str() : "null ctx"; }
int zkp_set_validate(zkp_ctx* c, int on) { if (!c) return ZKP_ERR_ARG; c->validate = on ? 1 : 0; return ZKP_OK; }
int zkp_set_kernel(zkp_ctx* c, int kind) {
    if (!c || kind < ZKP_KERNEL_AUTO || kind > ZKP_KERNEL_COOP) return ZKP_ERR_ARG;
    if (kind == ZKP_KERNEL_COOP && !c->coop.available) { c->err = "cooperative kernels not available"; return ZKP_ERR_ARG; }
    c->kernel = kind;
    return ZKP_OK;
}
int zkp_device_info(const zkp_ctx* c, int* cus, int* clock_khz, char* name, size_t name_len) {
    if (!c) return ZKP_ERR_ARG;
    if (cus) *cus = c->prop.multiProcessorCount;
    if (clock_khz) *clock_khz = c->prop.clockRate;
    if (name && name_len) { strncpy(name, c->prop.gcnArchName, name_len - 1); name[name_len - 1] = 0; }
    return ZKP_OK;
}

// ---------------------------------------------------------------- device-pointer API
#define S(stream) ((hipStream_t)(stream))
namespace {
// The workspace inside a ctx (line buffers, per-check state, product tree, flags) is shared by every call: a *_dev call
// first makes its stream wait for the previous call's last use of the workspace - which may have been queued on ANOTHER
// stream - and leaves an event behind for the next one.  Calls on one stream order themselves anyway.
// A stream that is being CAPTURED into a hipGraph (round 6) takes no part in that hand-over: an event recorded outside the capture may
// not be waited for inside it, and one recorded inside would poison the next ordinary call.  Whoever replays the graph orders it
// against the context's other calls himself (one stream, or his own events) - include/zkp_pairings.h, "hipGraph capture".
struct DevCall {
    zkp_ctx* c;
    hipStream_t s;
    int rc;
    bool capturing;
    DevCall(zkp_ctx* ctx, void* stream) : c(ctx), s((hipStream_t)stream), rc(ZKP_OK), capturing(false) {
        hipError_t e = hipSetDevice(c->device);
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (e == hipSuccess && s && hipStreamIsCapturing(s, &cs) == hipSuccess) capturing = cs == hipStreamCaptureStatusActive;
        if (e == hipSuccess && !capturing) e = hipStreamWaitEvent(s, c->ws_busy, 0);
        if (e != hipSuccess) { c->err = std::string("DevCall: ") + hipGetErrorString(e); rc = ZKP_ERR_HIP; }
    }
    ~DevCall() { if (rc == ZKP_OK && !capturing) (void)hipEventRecord(c->ws_busy, s); }
};
// validation mode on the device-pointer entry points: a range check of the inputs on the caller's stream that ORs into a
// sticky word (no host synchronisation); zkp_take_validation_status_dev reads and clears it
int validate_on_stream(zkp_ctx* c, const void* d, size_t n_fp, hipStream_t s) {
    if (!c->validate || !n_fp || !d) return ZKP_OK;
    hipLaunchKernelGGL(k_check_canonical, dim3(grid_for(n_fp, 256)), dim3(256), 0, s, (const uint64_t*)d, n_fp, c->d_flag + 2);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}
// ... of the G1 and G2 points of n pairs
int validate_pairs_on_stream(zkp_ctx* c, const void* g1, const void* g2, size_t n, hipStream_t s) {
    const int rc = validate_on_stream(c, g1, n * 2, s);
    return rc ? rc : validate_on_stream(c, g2, n * 4, s);
}
}  // namespace
#define DEV_ENTER(ctx, stream)      \
    DevCall dc__((ctx), (stream)); \
    if (dc__.rc) return dc__.rc
// range limits shared by the entry points: every per-launch count stays in 32 bits
using zkp::plan::too_many;   // zkp_plan.hpp: n <= 2^31 - 1, k <= 65535, n * k <= 2^31 - 1

int zkp_pairing_batch_dev(zkp_ctx* c, const void* g1, const void* g2, const void* i1, const void* i2, size_t n, void* out, void* stream) {
    if (!c || too_many(n) || (n && (!g1 || !g2 || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_pairs_on_stream(c, g1, g2, n, S(stream))) return rc;
    return pairing_dev(c, (const uint64_t*)g1, (const uint64_t*)g2, (const uint8_t*)i1, (const uint8_t*)i2, n, 1, (uint64_t*)out, nullptr, nullptr, S(stream));
}
int zkp_multi_miller_loop_batch_dev(zkp_ctx* c, const void* g1, const void* g2, const void* i1, const void* i2, size_t n_checks, size_t k,
                                    void* out, void* stream) {
    if (!c || too_many(n_checks, k) || (n_checks && (!out || (k && (!g1 || !g2))))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_pairs_on_stream(c, g1, g2, n_checks * k, S(stream))) return rc;
    return miller_dev(c, (const uint64_t*)g1, (const uint64_t*)g2, (const uint8_t*)i1, (const uint8_t*)i2, n_checks, k, (uint64_t*)out, S(stream));
}
int zkp_final_exponentiation_batch_dev(zkp_ctx* c, const void* f, size_t n, void* out, void* stream) {
    if (!c || too_many(n) || (n && (!f || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, f, n * 12, S(stream))) return rc;
    return final_exp_dev(c, (const uint64_t*)f, n, (uint64_t*)out, S(stream));
}
int zkp_fp12_product_dev(zkp_ctx* c, const void* f, size_t n, void* out, void* stream) {
    if (!c || !out || (n && !f) || too_many(n)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, f, n * 12, S(stream))) return rc;
    return fp12_product_dev(c, (const uint64_t*)f, n, (uint64_t*)out, S(stream));
}
int zkp_miller_product_dev(zkp_ctx* c, const void* g1, const void* g2, const void* i1, const void* i2, size_t n, void* out_ml, void* stream) {
    if (!c || !out_ml || (n && (!g1 || !g2)) || too_many(n)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_pairs_on_stream(c, g1, g2, n, S(stream))) return rc;
    return miller_product_dev(c, (const uint64_t*)g1, (const uint64_t*)g2, (const uint8_t*)i1, (const uint8_t*)i2, n, (uint64_t*)out_ml, S(stream));
}
int zkp_pairing_product_check_dev(zkp_ctx* c, const void* g1, const void* g2, const void* i1, const void* i2, size_t n, void* out_gt,
                                  void* is_one, void* stream) {
    if (!c || (n && (!g1 || !g2)) || too_many(n)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_pairs_on_stream(c, g1, g2, n, S(stream))) return rc;
    return product_check_dev(c, (const uint64_t*)g1, (const uint64_t*)g2, (const uint8_t*)i1, (const uint8_t*)i2, n, (uint64_t*)out_gt, (int*)is_one,
                             S(stream));
}
int zkp_pairing_check_batch_dev(zkp_ctx* c, const void* g1, const void* g2, const void* i1, const void* i2, size_t n_checks, size_t k,
                                void* ok, void* all_ok, void* stream) {
    if (!c || too_many(n_checks, k) || (n_checks && k && (!g1 || !g2))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_pairs_on_stream(c, g1, g2, n_checks * k, S(stream))) return rc;
    return pairing_dev(c, (const uint64_t*)g1, (const uint64_t*)g2, (const uint8_t*)i1, (const uint8_t*)i2, n_checks, k, nullptr, (uint8_t*)ok,
                       (int*)all_ok, S(stream));
}
int zkp_pairing_gt_check_batch_dev(zkp_ctx* c, const void* g1, const void* g2, const void* i1, const void* i2, size_t n_checks, size_t k,
                                   void* out_gt, void* ok, void* all_ok, void* stream) {
    if (!c || too_many(n_checks, k) || (n_checks && k && (!g1 || !g2))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_pairs_on_stream(c, g1, g2, n_checks * k, S(stream))) return rc;
    return pairing_dev(c, (const uint64_t*)g1, (const uint64_t*)g2, (const uint8_t*)i1, (const uint8_t*)i2, n_checks, k, (uint64_t*)out_gt,
                       (uint8_t*)ok, (int*)all_ok, S(stream));
}
// is_valid of n G1 (which = 1) or G2 (which = 2) points on the context's kernel family, on stream s
static int valid_dev(zkp_ctx* c, int which, const void* pts, const void* inf, size_t n, void* status, hipStream_t s) {
    if (!n) return ZKP_OK;
    if (zkp::coop_selected(&c->coop, c->kernel)) {
        HIPCHK(c, which == 1 ? zkp::coop_g1_valid((const uint64_t*)pts, (const uint8_t*)inf, n, (uint8_t*)status, s)
                             : zkp::coop_g2_valid(&c->coop, (const uint64_t*)pts, (const uint8_t*)inf, n, (uint8_t*)status, s));
        return ZKP_OK;
    }
    if (which == 1)
        hipLaunchKernelGGL(k_g1_valid, dim3(grid_for(n, TPB)), dim3(TPB), 0, s, (const uint64_t*)pts, (const uint8_t*)inf, n, (uint8_t*)status);
    else
        hipLaunchKernelGGL(k_g2_valid, dim3(grid_for(n, TPB)), dim3(TPB), 0, s, (const uint64_t*)pts, (const uint8_t*)inf, n, (uint8_t*)status);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}
int zkp_g1_is_valid_batch_dev(zkp_ctx* c, const void* g1, const void* inf, size_t n, void* status, void* stream) {
    if (!c || too_many(n) || (n && (!g1 || !status))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    if (int rc = validate_on_stream(c, g1, n * 2, S(stream))) return rc;
    return valid_dev(c, 1, g1, inf, n, status, S(stream));
}
int zkp_g2_is_valid_batch_dev(zkp_ctx* c, const void* g2, const void* inf, size_t n, void* status, void* stream) {
    if (!c || too_many(n) || (n && (!g2 || !status))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    if (int rc = validate_on_stream(c, g2, n * 4, S(stream))) return rc;
    return valid_dev(c, 2, g2, inf, n, status, S(stream));
}
// ---- point codecs on resident buffers: uncompressed (96 / 192 B per G1 / G2 point, round 4: the decode / encode kernels above) or
// compressed (48 / 96 B, zkp_compress.hip).  decode: bytes -> points, infinity flags, status bytes; encode: points (+ flags) -> bytes
static int codec_dev(zkp_ctx* c, bool compressed, bool decode, int which, const void* in, const void* inf_in, size_t n, void* out, void* out_inf,
                     void* status, hipStream_t s) {
    if (!n) return ZKP_OK;
    if (compressed)
        return decode ? coop_rc(c, which == 1 ? "g1_decompress" : "g2_decompress", zkp_cmp::decompress(which, in, n, out, out_inf, status, s))
                      : coop_rc(c, which == 1 ? "g1_compress" : "g2_compress", zkp_cmp::compress(which, in, inf_in, n, out, s));
    const int nfp = 2 * which;
    const bool aligned = (((uintptr_t)in | (uintptr_t)out) & 7u) == 0;
    if (decode) {
        if (aligned)
            hipLaunchKernelGGL(k_decode<true>, dim3(grid_for(n, 256)), dim3(256), 0, s, (const uint8_t*)in, n, nfp, (uint64_t*)out, (uint8_t*)out_inf, (uint8_t*)status);
        else
            hipLaunchKernelGGL(k_decode<false>, dim3(grid_for(n, 256)), dim3(256), 0, s, (const uint8_t*)in, n, nfp, (uint64_t*)out, (uint8_t*)out_inf, (uint8_t*)status);
    } else {
        if (aligned)
            hipLaunchKernelGGL(k_encode<true>, dim3(grid_for(n, 256)), dim3(256), 0, s, (const uint64_t*)in, (const uint8_t*)inf_in, n, nfp, (uint8_t*)out);
        else
            hipLaunchKernelGGL(k_encode<false>, dim3(grid_for(n, 256)), dim3(256), 0, s, (const uint64_t*)in, (const uint8_t*)inf_in, n, nfp, (uint8_t*)out);
    }
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}
int zkp_g1_decode_batch_dev(zkp_ctx* c, const void* bytes, size_t n, void* out_g1, void* out_inf, void* status, void* stream) {
    if (!c || too_many(n) || (n && (!bytes || !out_g1 || !out_inf || !status))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return codec_dev(c, false, true, 1, bytes, nullptr, n, out_g1, out_inf, status, S(stream));
}
int zkp_g2_decode_batch_dev(zkp_ctx* c, const void* bytes, size_t n, void* out_g2, void* out_inf, void* status, void* stream) {
    if (!c || too_many(n) || (n && (!bytes || !out_g2 || !out_inf || !status))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return codec_dev(c, false, true, 2, bytes, nullptr, n, out_g2, out_inf, status, S(stream));
}
int zkp_g1_encode_batch_dev(zkp_ctx* c, const void* g1, const void* inf, size_t n, void* out_bytes, void* stream) {
    if (!c || too_many(n) || (n && (!g1 || !out_bytes))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return codec_dev(c, false, false, 1, g1, inf, n, out_bytes, nullptr, nullptr, S(stream));
}
int zkp_g2_encode_batch_dev(zkp_ctx* c, const void* g2, const void* inf, size_t n, void* out_bytes, void* stream) {
    if (!c || too_many(n) || (n && (!g2 || !out_bytes))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return codec_dev(c, false, false, 2, g2, inf, n, out_bytes, nullptr, nullptr, S(stream));
}

// ---- BASELINE config 5 as ONE call: raw uncompressed bytes -> decode -> is_valid -> pairing check, everything between the byte
// strings and the status / ok bytes resident in HBM (the context's workspace)
static int ensure_pc(zkp_ctx* c, int slot, size_t bytes) {
    if (bytes <= c->pc_cap[slot]) return ZKP_OK;
    if (c->pc[slot]) { HIPCHK(c, hipFree(c->pc[slot])); c->pc[slot] = nullptr; c->pc_cap[slot] = 0; }
    HIPCHK(c, hipMalloc(&c->pc[slot], bytes));
    zkp_dbg_alloc("ctx.pc", c->pc[slot], bytes);
    c->pc_cap[slot] = bytes;
    return ZKP_OK;
}
enum { PC_G1 = 0, PC_G2, PC_INF1, PC_INF2, PC_DEC, PC_VAL, PC_ST1, PC_ST2, PC_OK, PC_BYTES, PC_IDX, PC_CNT, PC_CG1, PC_CG2, PC_CINF1, PC_CINF2, PC_COK };
// Validate first, then use (reference src/g1.rs:49-62, src/g2.rs:57-69: is_valid before anything is done with a point): the checks whose
// points are all valid are listed on the device (wave-aggregated compaction), gathered next to each other, and only those enter the
// Miller loop and the final exponentiation - a check with an invalid point costs its validity tests and nothing else.  Round 6: the
// NUMBER of listed checks stays in device memory.  The pairing phase is planned for the worst case (every check valid) and its kernels
// read the count themselves (zkp::coop_pairing's n_dev: wavefronts behind the count leave at once), so the call never waits on the
// host: asynchronous on `s` like every other *_dev entry point, and capturable into a hipGraph once its workspaces exist.  (Round 5 read
// the count back - 4 bytes, one hipStreamSynchronize - to size the grids on the host.)  The thread family has no such kernels: it
// runs the fused pairing on every check and fails the invalid ones afterwards (k_checks_merge), as round 4 did.
// `compressed` picks the input format of the decode step: uncompressed (96 / 192 B per point, k_decode) or compressed (48 / 96 B per
// point, zkp_compress.hip - decompression status 3 is "not on the curve", which k_points_merge passes through as ZKP_POINT_NOT_ON_CURVE).
// Everything after the decode step is the same for both.
static int points_check_dev(zkp_ctx* c, const void* b1, const void* b2, size_t n_checks, size_t k, void* st1, void* st2, void* ok, int* all_ok,
                            hipStream_t s, bool compressed) {
    const size_t np = n_checks * k;
    const bool compact = n_checks && k && zkp::coop_selected(&c->coop, c->kernel) && zkp::coop_supports_k(k);
    int rc;
    // every workspace first (an allocation synchronises the device): nothing below this block allocates
    if ((rc = ensure_pc(c, PC_G1, np * 96 + 8)) || (rc = ensure_pc(c, PC_G2, np * 192 + 8)) || (rc = ensure_pc(c, PC_INF1, np + 8)) ||
        (rc = ensure_pc(c, PC_INF2, np + 8)) || (rc = ensure_pc(c, PC_DEC, 2 * np + 8)) || (rc = ensure_pc(c, PC_VAL, 2 * np + 8)) ||
        (rc = ensure_pc(c, PC_ST1, np + 8)) || (rc = ensure_pc(c, PC_ST2, np + 8)) || (rc = ensure_pc(c, PC_OK, n_checks + 8)))
        return rc;
    if (compact && ((rc = ensure_pc(c, PC_IDX, n_checks * 4 + 8)) || (rc = ensure_pc(c, PC_CNT, 8)) || (rc = ensure_pc(c, PC_CG1, np * 96 + 8)) ||
                    (rc = ensure_pc(c, PC_CG2, np * 192 + 8)) || (rc = ensure_pc(c, PC_CINF1, np + 8)) || (rc = ensure_pc(c, PC_CINF2, np + 8)) ||
                    (rc = ensure_pc(c, PC_COK, n_checks + 8))))
        return rc;
    uint8_t* dec1 = (uint8_t*)c->pc[PC_DEC];
    uint8_t* dec2 = dec1 + np;
    uint8_t* val1 = (uint8_t*)c->pc[PC_VAL];
    uint8_t* val2 = val1 + np;
    uint8_t* s1 = st1 ? (uint8_t*)st1 : (uint8_t*)c->pc[PC_ST1];
    uint8_t* s2 = st2 ? (uint8_t*)st2 : (uint8_t*)c->pc[PC_ST2];
    uint8_t* okb = ok ? (uint8_t*)ok : (uint8_t*)c->pc[PC_OK];
    if (np) {
        if ((rc = codec_dev(c, compressed, true, 1, b1, nullptr, np, c->pc[PC_G1], c->pc[PC_INF1], dec1, s)) ||
            (rc = codec_dev(c, compressed, true, 2, b2, nullptr, np, c->pc[PC_G2], c->pc[PC_INF2], dec2, s)))
            return rc;
        if ((rc = valid_dev(c, 1, c->pc[PC_G1], c->pc[PC_INF1], np, val1, s)) || (rc = valid_dev(c, 2, c->pc[PC_G2], c->pc[PC_INF2], np, val2, s)))
            return rc;
        hipLaunchKernelGGL(k_points_merge, dim3(grid_for(np, 256)), dim3(256), 0, s, dec1, val1, (uint8_t*)c->pc[PC_INF1], np, s1);
        hipLaunchKernelGGL(k_points_merge, dim3(grid_for(np, 256)), dim3(256), 0, s, dec2, val2, (uint8_t*)c->pc[PC_INF2], np, s2);
        HIPCHK(c, hipGetLastError());
    }
    if (!compact) {
        if ((rc = pairing_dev(c, (const uint64_t*)c->pc[PC_G1], (const uint64_t*)c->pc[PC_G2], (const uint8_t*)c->pc[PC_INF1], (const uint8_t*)c->pc[PC_INF2],
                              n_checks, k, nullptr, okb, all_ok, s)))
            return rc;
        if (n_checks && k) {
            hipLaunchKernelGGL(k_checks_merge, dim3(grid_for(n_checks, 256)), dim3(256), 0, s, s1, s2, n_checks, k, okb, all_ok);
            HIPCHK(c, hipGetLastError());
        }
        return ZKP_OK;
    }
    uint32_t* const idx = (uint32_t*)c->pc[PC_IDX];
    uint32_t* const cnt = (uint32_t*)c->pc[PC_CNT];
    HIPCHK(c, hipMemsetAsync(cnt, 0, 4, s));
    hipLaunchKernelGGL(k_checks_compact, dim3(grid_for(n_checks, 256)), dim3(256), 0, s, s1, s2, n_checks, k, idx, cnt, okb);
    hipLaunchKernelGGL(k_gather_checks<uint64_t>, dim3(grid_for(np * 12, 256)), dim3(256), 0, s, (const uint64_t*)c->pc[PC_G1], idx, cnt, n_checks, k * 12, (uint64_t*)c->pc[PC_CG1]);
    hipLaunchKernelGGL(k_gather_checks<uint64_t>, dim3(grid_for(np * 24, 256)), dim3(256), 0, s, (const uint64_t*)c->pc[PC_G2], idx, cnt, n_checks, k * 24, (uint64_t*)c->pc[PC_CG2]);
    hipLaunchKernelGGL(k_gather_checks<uint8_t>, dim3(grid_for(np, 256)), dim3(256), 0, s, (const uint8_t*)c->pc[PC_INF1], idx, cnt, n_checks, k, (uint8_t*)c->pc[PC_CINF1]);
    hipLaunchKernelGGL(k_gather_checks<uint8_t>, dim3(grid_for(np, 256)), dim3(256), 0, s, (const uint8_t*)c->pc[PC_INF2], idx, cnt, n_checks, k, (uint8_t*)c->pc[PC_CINF2]);
    HIPCHK(c, hipGetLastError());
    // the listed checks (their points are all valid): fused pairing, ok bytes in list order, the AND flag over them
    if ((rc = pairing_dev(c, (const uint64_t*)c->pc[PC_CG1], (const uint64_t*)c->pc[PC_CG2], (const uint8_t*)c->pc[PC_CINF1], (const uint8_t*)c->pc[PC_CINF2],
                          n_checks, k, nullptr, (uint8_t*)c->pc[PC_COK], all_ok, s, true, cnt)))
        return rc;
    hipLaunchKernelGGL(k_scatter_ok, dim3(grid_for(n_checks, 256)), dim3(256), 0, s, (const uint8_t*)c->pc[PC_COK], idx, cnt, n_checks, okb);
    if (all_ok) hipLaunchKernelGGL(k_flag_if_fewer, dim3(1), dim3(1), 0, s, all_ok, cnt, (uint32_t)n_checks);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}
int zkp_points_check_batch_dev(zkp_ctx* c, const void* g1_bytes, const void* g2_bytes, size_t n_checks, size_t k, void* st1, void* st2, void* ok,
                               void* all_ok, void* stream) {
    if (!c || too_many(n_checks, k) || (n_checks && k && (!g1_bytes || !g2_bytes))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return points_check_dev(c, g1_bytes, g2_bytes, n_checks, k, st1, st2, ok, (int*)all_ok, S(stream), false);
}
int zkp_points_check_compressed_batch_dev(zkp_ctx* c, const void* g1_bytes, const void* g2_bytes, size_t n_checks, size_t k, void* st1, void* st2,
                                          void* ok, void* all_ok, void* stream) {
    if (!c || too_many(n_checks, k) || (n_checks && k && (!g1_bytes || !g2_bytes))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return points_check_dev(c, g1_bytes, g2_bytes, n_checks, k, st1, st2, ok, (int*)all_ok, S(stream), true);
}

// ---- compressed point codec on resident buffers (zkp_compress.hip): 48 B per G1 point, 96 B per G2 point
int zkp_g1_decompress_batch_dev(zkp_ctx* c, const void* bytes, size_t n, void* out_g1, void* out_inf, void* status, void* stream) {
    if (!c || too_many(n) || (n && (!bytes || !out_g1 || !out_inf || !status))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return codec_dev(c, true, true, 1, bytes, nullptr, n, out_g1, out_inf, status, S(stream));
}
int zkp_g2_decompress_batch_dev(zkp_ctx* c, const void* bytes, size_t n, void* out_g2, void* out_inf, void* status, void* stream) {
    if (!c || too_many(n) || (n && (!bytes || !out_g2 || !out_inf || !status))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return codec_dev(c, true, true, 2, bytes, nullptr, n, out_g2, out_inf, status, S(stream));
}
int zkp_g1_compress_batch_dev(zkp_ctx* c, const void* g1, const void* inf, size_t n, void* out_bytes, void* stream) {
    if (!c || too_many(n) || (n && (!g1 || !out_bytes))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return codec_dev(c, true, false, 1, g1, inf, n, out_bytes, nullptr, nullptr, S(stream));
}
int zkp_g2_compress_batch_dev(zkp_ctx* c, const void* g2, const void* inf, size_t n, void* out_bytes, void* stream) {
    if (!c || too_many(n) || (n && (!g2 || !out_bytes))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return codec_dev(c, true, false, 2, g2, inf, n, out_bytes, nullptr, nullptr, S(stream));
}

// [sc_i] base_i of n G1 (which = 1) or G2 (which = 2) points; stride 0: one base point for every scalar
static int mul_dev(zkp_ctx* c, int which, const void* base, size_t stride, const void* sc, size_t n, void* out, void* out_inf, hipStream_t s) {
    if (zkp::coop_selected(&c->coop, c->kernel)) {
        HIPCHK(c, which == 1 ? zkp::coop_g1_mul((const uint64_t*)base, stride, (const uint64_t*)sc, n, (uint64_t*)out, (uint8_t*)out_inf, s)
                             : zkp::coop_g2_mul((const uint64_t*)base, stride, (const uint64_t*)sc, n, (uint64_t*)out, (uint8_t*)out_inf, s));
        return ZKP_OK;
    }
    if (which == 1)
        hipLaunchKernelGGL(k_g1_mul, dim3(grid_for(n, TPB)), dim3(TPB), 0, s, (const uint64_t*)base, stride, (const uint64_t*)sc, n, (uint64_t*)out, (uint8_t*)out_inf);
    else
        hipLaunchKernelGGL(k_g2_mul, dim3(grid_for(n, TPB)), dim3(TPB), 0, s, (const uint64_t*)base, stride, (const uint64_t*)sc, n, (uint64_t*)out, (uint8_t*)out_inf);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}
int zkp_g1_mul_batch_dev(zkp_ctx* c, const void* base, size_t stride, const void* sc, size_t n, void* out, void* out_inf, void* stream) {
    if (!c || too_many(n) || (n && (!base || !sc || !out)) || (stride != 0 && stride != 12)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    if (int rc = validate_on_stream(c, base, (stride ? n : 1) * 2, S(stream))) return rc;
    return mul_dev(c, 1, base, stride, sc, n, out, out_inf, S(stream));
}
int zkp_g2_mul_batch_dev(zkp_ctx* c, const void* base, size_t stride, const void* sc, size_t n, void* out, void* out_inf, void* stream) {
    if (!c || too_many(n) || (n && (!base || !sc || !out)) || (stride != 0 && stride != 24)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    if (int rc = validate_on_stream(c, base, (stride ? n : 1) * 4, S(stream))) return rc;
    return mul_dev(c, 2, base, stride, sc, n, out, out_inf, S(stream));
}

// ---- group addition and multi-scalar multiplication (28-bit core whatever zkp_set_kernel says)
static int add_dev(zkp_ctx* c, int which, const void* a, const void* ia, const void* b, const void* ib, size_t n, void* out, void* out_inf, hipStream_t s) {
    return coop_rc(c, which == 1 ? "g1_add" : "g2_add",
                   zkp::coop_add(which, (const uint64_t*)a, (const uint8_t*)ia, (const uint64_t*)b, (const uint8_t*)ib, n, (uint64_t*)out, (uint8_t*)out_inf, s));
}
int zkp_g1_add_batch_dev(zkp_ctx* c, const void* a, const void* inf_a, const void* b, const void* inf_b, size_t n, void* out, void* out_inf, void* stream) {
    if (!c || too_many(n) || (n && (!a || !b || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    int rc;
    if ((rc = validate_on_stream(c, a, n * 2, S(stream))) || (rc = validate_on_stream(c, b, n * 2, S(stream)))) return rc;
    return add_dev(c, 1, a, inf_a, b, inf_b, n, out, out_inf, S(stream));
}
int zkp_g2_add_batch_dev(zkp_ctx* c, const void* a, const void* inf_a, const void* b, const void* inf_b, size_t n, void* out, void* out_inf, void* stream) {
    if (!c || too_many(n) || (n && (!a || !b || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    int rc;
    if ((rc = validate_on_stream(c, a, n * 4, S(stream))) || (rc = validate_on_stream(c, b, n * 4, S(stream)))) return rc;
    return add_dev(c, 2, a, inf_a, b, inf_b, n, out, out_inf, S(stream));
}
static int msm_grow(zkp_ctx* c, size_t bytes) {
    if (bytes <= c->msm_cap) return ZKP_OK;
    if (c->msm_ws) { HIPCHK(c, hipFree(c->msm_ws)); c->msm_ws = nullptr; c->msm_cap = 0; }
    if (hipMalloc(&c->msm_ws, bytes) != hipSuccess) { c->msm_ws = nullptr; c->err = "msm: workspace allocation"; return ZKP_ERR_OOM; }
    zkp_dbg_alloc("ctx.msm", c->msm_ws, bytes);
    c->msm_cap = bytes;
    return ZKP_OK;
}
// n_msm >= 1 sums; grows the context's MSM workspace (an allocation synchronises the device) before it queues anything
static int msm_dev(zkp_ctx* c, int which, const void* pts, const void* inf, const void* sc, size_t m, size_t n_msm, int shared, void* out, void* out_inf,
                   hipStream_t s, float* phase_ms) {
    const size_t bytes = zkp::msm_workspace_bytes(which, m, n_msm, shared);
    if (!bytes) { c->err = "msm: workspace size"; return ZKP_ERR_ARG; }
    if (int rc = msm_grow(c, bytes)) return rc;
    return coop_rc(c, which == 1 ? "g1_msm" : "g2_msm",
                   zkp::msm_run(which, c->msm_ws, (const uint64_t*)pts, (const uint8_t*)inf, (const uint64_t*)sc, m, n_msm, shared ? 1 : 0, (uint64_t*)out,
                                (uint8_t*)out_inf, s, phase_ms));
}
int zkp_g1_msm_batch_dev(zkp_ctx* c, const void* points, const void* inf, const void* scalars, size_t m, size_t n_msm, int shared_bases, void* out,
                         void* out_inf, void* stream) {
    if (!c || zkp::msm::msm_args_bad(m, n_msm) || (n_msm && (!points || !scalars || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n_msm) return ZKP_OK;
    if (int rc = validate_on_stream(c, points, (shared_bases ? m : m * n_msm) * 2, S(stream))) return rc;
    return msm_dev(c, 1, points, inf, scalars, m, n_msm, shared_bases, out, out_inf, S(stream), nullptr);
}
int zkp_g2_msm_batch_dev(zkp_ctx* c, const void* points, const void* inf, const void* scalars, size_t m, size_t n_msm, int shared_bases, void* out,
                         void* out_inf, void* stream) {
    if (!c || zkp::msm::msm_args_bad(m, n_msm) || (n_msm && (!points || !scalars || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n_msm) return ZKP_OK;
    if (int rc = validate_on_stream(c, points, (shared_bases ? m : m * n_msm) * 4, S(stream))) return rc;
    return msm_dev(c, 2, points, inf, scalars, m, n_msm, shared_bases, out, out_inf, S(stream), nullptr);
}
int zkp_msm_profile_dev(zkp_ctx* c, int which, const void* points, const void* inf, const void* scalars, size_t m, size_t n_msm, int shared_bases,
                        void* out, void* out_inf, void* stream, float* phase_ms) {
    if (!phase_ms || (which != 1 && which != 2)) return ZKP_ERR_ARG;
    for (int i = 0; i < zkp::MSM_PHASES; i++) phase_ms[i] = 0;
    if (!c || zkp::msm::msm_args_bad(m, n_msm) || (n_msm && (!points || !scalars || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n_msm) return ZKP_OK;
    if (int rc = validate_on_stream(c, points, (shared_bases ? m : m * n_msm) * 2 * which, S(stream))) return rc;
    return msm_dev(c, which, points, inf, scalars, m, n_msm, shared_bases, out, out_inf, S(stream), phase_ms);
}

// ---- batch verification by random linear combination (zkp_rlc.hip drives it; 28-bit core for the scaling, the context's family for
// the pairing)
static int endo_dev(zkp_ctx* c, const void* base, const void* inf, const void* ab, size_t n, void* out, void* out_inf, hipStream_t s) {
    return coop_rc(c, "g1_mul_endo",
                   zkp::coop_g1_mul_endo((const uint64_t*)base, (const uint8_t*)inf, (const uint64_t*)ab, n, 1, (uint64_t*)out, (uint8_t*)out_inf, s));
}
int zkp_g1_mul_endo_batch_dev(zkp_ctx* c, const void* base, const void* inf, const void* ab, size_t n, void* out, void* out_inf, void* stream) {
    if (!c || too_many(n) || (n && (!base || !ab || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    if (int rc = validate_on_stream(c, base, n * 2, S(stream))) return rc;
    return endo_dev(c, base, inf, ab, n, out, out_inf, S(stream));
}
// the argument check of both flavours (zkp_rlc_plan.hpp: the size limits)
static bool rlc_args_bad(const zkp_ctx* c, const zkp_rlc_batch* b, const void* rand, int flags, const void* all_ok) {
    if (!c || !b || !all_ok || (flags & ~ZKP_RLC_POINTS_CHECKED) || zkp::rlc::args_bad(b->n_checks, b->k, b->s1, b->s2)) return true;
    if (!b->n_checks) return false;
    return !rand || (b->k && (!b->g1 || !b->g2)) || (b->s2 && (!b->col_g1 || !b->fixed_g2)) || (b->s1 && (!b->col_g2 || !b->fixed_g1));
}
// validation mode: v(pointer, Fp count) over every coordinate array of the batch
extern "C++" template <class V>
static int rlc_validate(const zkp_rlc_batch* b, V&& v) {
    const size_t n = b->n_checks;
    int rc;
    if ((rc = v(b->g1, n * b->k * 2)) || (rc = v(b->g2, n * b->k * 4)) || (rc = v(b->col_g1, n * b->s2 * 2)) || (rc = v(b->fixed_g2, b->s2 * 4)) ||
        (rc = v(b->col_g2, n * b->s1 * 4)) || (rc = v(b->fixed_g1, b->s1 * 2)))
        return rc;
    return ZKP_OK;
}
int zkp_pairing_check_batch_rlc_dev(zkp_ctx* c, const zkp_rlc_batch* b, const void* rand, int flags, void* all_ok, void* stream) {
    if (rlc_args_bad(c, b, rand, flags, all_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (b->n_checks)
        if (int rc = rlc_validate(b, [&](const void* d, size_t n_fp) { return validate_on_stream(c, d, n_fp, S(stream)); })) return rc;
    return zkp::rlc_check_dev(c, b, (const uint64_t*)rand, flags, (int*)all_ok, S(stream));
}

// validation mode of the device-pointer entry points: *bad = 1 if any *_dev call since the last query saw a field
// element >= p in its inputs (the results of such a call are unspecified).  Waits for `stream`, then clears the word.
int zkp_take_validation_status_dev(zkp_ctx* c, void* stream, int* bad) {
    if (!c || !bad) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, c->d_flag + 2, sizeof(int), hipMemcpyDeviceToHost, S(stream)));
    HIPCHK(c, hipMemsetAsync(c->d_flag + 2, 0, sizeof(int), S(stream)));
    HIPCHK(c, hipStreamSynchronize(S(stream)));
    *bad = v ? 1 : 0;
    return ZKP_OK;
}

// ---------------------------------------------------------------- host-pointer API
// Each call: argument checks, its inputs staged in the context's workspace (HostIO), the inputs range-checked in validation mode
// (validate_dev), the same launch-only function as the *_dev flavour on the context's stream, the downloads and one synchronisation.
int zkp_pairing_batch(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n, uint64_t* out_gt) {
    if (!c || (n && (!g1 || !g2 || !out_gt))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    int rc;
    if ((rc = io.status())) return rc;
    if (n > c->host_slice && !c->validate) return host_sliced(c, g1, g2, inf1, inf2, n, 1, out_gt, nullptr, nullptr);
    Staged st;
    if ((rc = stage_pairs(io, g1, g2, inf1, inf2, n, &st))) return rc;
    void* gt = io.out(4, out_gt, n * 576);
    if ((rc = io.status()) || (rc = pairing_dev(c, st.g1, st.g2, st.i1, st.i2, n, 1, (uint64_t*)gt, nullptr, nullptr, c->stream))) return rc;
    return io.finish();
}
int zkp_multi_miller_loop_batch(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n_checks,
                                size_t k, uint64_t* out_ml) {
    if (!c || (n_checks && (!out_ml || (k && (!g1 || !g2))))) return ZKP_ERR_ARG;
    if (!n_checks) return ZKP_OK;
    HostIO io(c);
    Staged st = {nullptr, nullptr, nullptr, nullptr};
    int rc;
    if (k && (rc = stage_pairs(io, g1, g2, inf1, inf2, n_checks * k, &st))) return rc;
    void* out = io.out(4, out_ml, n_checks * 576);
    if ((rc = io.status()) || (rc = miller_dev(c, st.g1, st.g2, st.i1, st.i2, n_checks, k, (uint64_t*)out, c->stream))) return rc;
    return io.finish();
}
int zkp_final_exponentiation_batch(zkp_ctx* c, const uint64_t* f, size_t n, uint64_t* out_gt) {
    if (!c || (n && (!f || !out_gt))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const uint64_t* df = (const uint64_t*)io.in(5, f, n * 576);
    void* out = io.out(4, out_gt, n * 576);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, df, n * 12)) || (rc = final_exp_dev(c, df, n, (uint64_t*)out, c->stream))) return rc;
    return io.finish();
}
int zkp_fp12_product(zkp_ctx* c, const uint64_t* f, size_t n, uint64_t* out) {
    if (!c || !out || (n && !f) || n > 0x7fffffffu) return ZKP_ERR_ARG;
    if (!n) { memcpy(out, GT_IDENTITY, 576); return ZKP_OK; }
    HostIO io(c);
    int rc;
    if ((rc = io.status()) || (rc = ensure_prod(c, n))) return rc;
    io.put(c->prod, f, n * 576);
    io.get(out, c->prod, 576);
    if ((rc = io.status()) || (rc = validate_dev(c, c->prod, n * 12)) || (rc = fp12_product_inplace(c, c->prod, n, c->stream))) return rc;
    return io.finish();
}
int zkp_miller_product(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n, uint64_t* out_ml) {
    if (!c || !out_ml || (n && (!g1 || !g2)) || n > 0x7fffffffu) return ZKP_ERR_ARG;
    if (!n) { memcpy(out_ml, GT_IDENTITY, 576); return ZKP_OK; }
    HostIO io(c);
    Staged st;
    int rc;
    if ((rc = stage_pairs(io, g1, g2, inf1, inf2, n, &st)) || (rc = miller_product_dev(c, st.g1, st.g2, st.i1, st.i2, n, nullptr, c->stream))) return rc;
    io.get(out_ml, c->prod, 576);   // the product tree's root (ensure_prod may have moved the tree)
    return io.finish();
}
int zkp_pairing_product_check(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n,
                              uint64_t* out_gt, int* is_one) {
    if (!c || (n && (!g1 || !g2)) || n > 0x7fffffffu) return ZKP_ERR_ARG;
    if (!n) {
        if (out_gt) memcpy(out_gt, GT_IDENTITY, 576);
        if (is_one) *is_one = 1;
        return ZKP_OK;
    }
    HostIO io(c);
    Staged st;
    int rc;
    if ((rc = stage_pairs(io, g1, g2, inf1, inf2, n, &st))) return rc;
    void* gt = io.out(4, out_gt, 576);
    io.get(is_one, c->d_flag, sizeof(int));
    if ((rc = io.status()) || (rc = product_check_dev(c, st.g1, st.g2, st.i1, st.i2, n, (uint64_t*)gt, c->d_flag, c->stream))) return rc;
    return io.finish();
}
int zkp_pairing_check_batch(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n_checks,
                            size_t k, uint8_t* ok, int* all_ok) {
    if (!c || (n_checks && k && (!g1 || !g2))) return ZKP_ERR_ARG;
    if (all_ok) *all_ok = 1;
    if (!n_checks) return ZKP_OK;
    HostIO io(c);
    int rc;
    if ((rc = io.status())) return rc;
    // flags-only results need no large download: one shot is faster (measured) until the upload workspace gets large
    if (k && n_checks * k > 8 * c->host_slice && !c->validate) return host_sliced(c, g1, g2, inf1, inf2, n_checks, k, nullptr, ok, all_ok);
    Staged st = {nullptr, nullptr, nullptr, nullptr};
    if (k && (rc = stage_pairs(io, g1, g2, inf1, inf2, n_checks * k, &st))) return rc;
    void* dok = io.out(6, ok, n_checks);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    if ((rc = io.status()) || (rc = pairing_dev(c, st.g1, st.g2, st.i1, st.i2, n_checks, k, nullptr, (uint8_t*)dok, c->d_flag + 1, c->stream))) return rc;
    return io.finish();
}
static int valid_host(zkp_ctx* c, int which, const uint64_t* pts, const uint8_t* inf, size_t n, uint8_t* status) {
    if (!c || too_many(n) || (n && (!pts || !status))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const uint64_t* dp = (const uint64_t*)io.in(0, pts, n * 96 * which);
    void* dst = io.out(6, status, n);
    const void* di = io.in(2, inf, n);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, dp, n * 2 * which)) || (rc = valid_dev(c, which, dp, di, n, dst, c->stream))) return rc;
    return io.finish();
}
int zkp_g1_is_valid_batch(zkp_ctx* c, const uint64_t* g1, const uint8_t* inf, size_t n, uint8_t* status) { return valid_host(c, 1, g1, inf, n, status); }
int zkp_g2_is_valid_batch(zkp_ctx* c, const uint64_t* g2, const uint8_t* inf, size_t n, uint8_t* status) { return valid_host(c, 2, g2, inf, n, status); }

// mul, add and MSM always hand their kernels the infinity-flag buffer (slot 6), whether or not the caller wants the flags
static int mul_host(zkp_ctx* c, int which, const uint64_t* base, size_t stride, const uint64_t* sc, size_t n, uint64_t* out, uint8_t* out_inf) {
    const size_t w = which == 1 ? 12 : 24;
    if (!c || too_many(n) || (n && (!base || !sc || !out)) || (stride != 0 && stride != w)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const size_t nb = stride ? n : 1;
    const uint64_t* db = (const uint64_t*)io.in(0, base, nb * w * 8);
    const void* ds = io.in(1, sc, n * 32);
    void* dout = io.out(4, out, n * w * 8);
    void* dinf = io.out(6, out_inf, n);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, db, nb * w / 6)) || (rc = mul_dev(c, which, db, stride, ds, n, dout, dinf, c->stream))) return rc;
    return io.finish();
}
int zkp_g1_mul_batch(zkp_ctx* c, const uint64_t* base, size_t stride, const uint64_t* sc, size_t n, uint64_t* out, uint8_t* out_inf) {
    return mul_host(c, 1, base, stride, sc, n, out, out_inf);
}
int zkp_g2_mul_batch(zkp_ctx* c, const uint64_t* base, size_t stride, const uint64_t* sc, size_t n, uint64_t* out, uint8_t* out_inf) {
    return mul_host(c, 2, base, stride, sc, n, out, out_inf);
}
static int add_host(zkp_ctx* c, int which, const uint64_t* a, const uint8_t* ia, const uint64_t* b, const uint8_t* ib, size_t n, uint64_t* out,
                    uint8_t* out_inf) {
    const size_t w = which == 1 ? 12 : 24;
    if (!c || too_many(n) || (n && (!a || !b || !out))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const uint64_t* da = (const uint64_t*)io.in(0, a, n * w * 8);
    const uint64_t* db = (const uint64_t*)io.in(1, b, n * w * 8);
    void* dout = io.out(4, out, n * w * 8);
    void* dinf = io.out(6, out_inf, n);
    const void* dia = io.in(2, ia, n);
    const void* dib = io.in(3, ib, n);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, da, n * w / 6)) || (rc = validate_dev(c, db, n * w / 6)) ||
        (rc = add_dev(c, which, da, dia, db, dib, n, dout, dinf, c->stream)))
        return rc;
    return io.finish();
}
int zkp_g1_add_batch(zkp_ctx* c, const uint64_t* a, const uint8_t* inf_a, const uint64_t* b, const uint8_t* inf_b, size_t n, uint64_t* out, uint8_t* out_inf) {
    return add_host(c, 1, a, inf_a, b, inf_b, n, out, out_inf);
}
int zkp_g2_add_batch(zkp_ctx* c, const uint64_t* a, const uint8_t* inf_a, const uint64_t* b, const uint8_t* inf_b, size_t n, uint64_t* out, uint8_t* out_inf) {
    return add_host(c, 2, a, inf_a, b, inf_b, n, out, out_inf);
}
static int msm_host(zkp_ctx* c, int which, const uint64_t* pts, const uint8_t* inf, const uint64_t* sc, size_t m, size_t n_msm, int shared, uint64_t* out,
                    uint8_t* out_inf) {
    const size_t w = which == 1 ? 12 : 24;
    if (!c || zkp::msm::msm_args_bad(m, n_msm) || (n_msm && (!pts || !sc || !out))) return ZKP_ERR_ARG;
    if (!n_msm) return ZKP_OK;
    HostIO io(c);
    const size_t terms = m * n_msm, np = shared ? m : terms;
    const uint64_t* dp = (const uint64_t*)io.in(0, pts, np * w * 8);
    const void* ds = io.in(1, sc, terms * 32);
    void* dout = io.out(4, out, n_msm * w * 8);
    void* dinf = io.out(6, out_inf, n_msm);
    const void* di = io.in(2, inf, np);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, dp, np * w / 6)) ||
        (rc = msm_dev(c, which, dp, di, ds, m, n_msm, shared, dout, dinf, c->stream, nullptr)))
        return rc;
    return io.finish();
}
int zkp_g1_msm_batch(zkp_ctx* c, const uint64_t* points, const uint8_t* inf, const uint64_t* scalars, size_t m, size_t n_msm, int shared_bases, uint64_t* out,
                     uint8_t* out_inf) {
    return msm_host(c, 1, points, inf, scalars, m, n_msm, shared_bases, out, out_inf);
}
int zkp_g2_msm_batch(zkp_ctx* c, const uint64_t* points, const uint8_t* inf, const uint64_t* scalars, size_t m, size_t n_msm, int shared_bases, uint64_t* out,
                     uint8_t* out_inf) {
    return msm_host(c, 2, points, inf, scalars, m, n_msm, shared_bases, out, out_inf);
}

}  // extern "C"

// what the RLC batch check (zkp_rlc.hip) borrows from the context: the same launch-only pieces the entry points above use
namespace zkp {
namespace ctxop {
int fail(zkp_ctx* c, const char* what, hipError_t e) { return coop_rc(c, what, e); }
int grow_rlc(zkp_ctx* c, size_t bytes, void** ws) {
    if (bytes > c->rlc_cap) {
        if (c->rlc_ws) { HIPCHK(c, hipFree(c->rlc_ws)); c->rlc_ws = nullptr; c->rlc_cap = 0; }
        HIPCHK(c, hipMalloc(&c->rlc_ws, bytes));
        zkp_dbg_alloc("ctx.rlc", c->rlc_ws, bytes);
        c->rlc_cap = bytes;
    }
    *ws = c->rlc_ws;
    return ZKP_OK;
}
int grow_g16(zkp_ctx* c, size_t bytes, void** ws) {
    if (bytes > c->g16_cap) {
        if (c->g16_ws) { HIPCHK(c, hipFree(c->g16_ws)); c->g16_ws = nullptr; c->g16_cap = 0; }
        HIPCHK(c, hipMalloc(&c->g16_ws, bytes));
        zkp_dbg_alloc("ctx.g16", c->g16_ws, bytes);
        c->g16_cap = bytes;
    }
    *ws = c->g16_ws;
    return ZKP_OK;
}
int grow_kzg(zkp_ctx* c, size_t bytes, void** ws) {
    if (bytes > c->kzg_cap) {
        if (c->kzg_ws) { HIPCHK(c, hipFree(c->kzg_ws)); c->kzg_ws = nullptr; c->kzg_cap = 0; }
        HIPCHK(c, hipMalloc(&c->kzg_ws, bytes));
        zkp_dbg_alloc("ctx.kzg", c->kzg_ws, bytes);
        c->kzg_cap = bytes;
    }
    *ws = c->kzg_ws;
    return ZKP_OK;
}
int kzg_domain(zkp_ctx* c, unsigned log2_n, const uint32_t** table, unsigned* table_log2, hipStream_t s) {
    if ((int)log2_n > c->kzg_dom_log2) {
        if (c->kzg_dom) { HIPCHK(c, hipFree(c->kzg_dom)); c->kzg_dom = nullptr; c->kzg_dom_log2 = -1; }
        HIPCHK(c, hipMalloc((void**)&c->kzg_dom, zkp::kzg::domain_bytes(log2_n)));
        zkp_dbg_alloc("ctx.kzg_dom", c->kzg_dom, zkp::kzg::domain_bytes(log2_n));
        HIPCHK(c, zkp::fr_domain_build(c->kzg_dom, log2_n, s));
        c->kzg_dom_log2 = (int)log2_n;
    }
    *table = c->kzg_dom;
    *table_log2 = (unsigned)c->kzg_dom_log2;
    return ZKP_OK;
}
int poly_coset(zkp_ctx* c, const uint32_t** coset, hipStream_t s) {
    if (!c->poly_coset) {
        HIPCHK(c, hipMalloc((void**)&c->poly_coset, zkp::poly::COSET_BYTES));
        zkp_dbg_alloc("ctx.poly_coset", c->poly_coset, zkp::poly::COSET_BYTES);
        const hipError_t e = zkp::poly_coset_build(c->poly_coset, s);
        if (e != hipSuccess) { (void)hipFree(c->poly_coset); c->poly_coset = nullptr; }
        HIPCHK(c, e);
    }
    *coset = c->poly_coset;
    return ZKP_OK;
}
int grow_prove(zkp_ctx* c, size_t bytes, void** ws) {
    if (bytes > c->prove_cap) {
        if (c->prove_ws) { HIPCHK(c, hipFree(c->prove_ws)); c->prove_ws = nullptr; c->prove_cap = 0; }
        HIPCHK(c, hipMalloc(&c->prove_ws, bytes));
        zkp_dbg_alloc("ctx.prove", c->prove_ws, bytes);
        c->prove_cap = bytes;
    }
    *ws = c->prove_ws;
    return ZKP_OK;
}
int grow_fk20(zkp_ctx* c, size_t bytes, void** ws) {
    if (bytes > c->fk20_cap) {
        if (c->fk20_ws) { HIPCHK(c, hipFree(c->fk20_ws)); c->fk20_ws = nullptr; c->fk20_cap = 0; }
        HIPCHK(c, hipMalloc(&c->fk20_ws, bytes));
        zkp_dbg_alloc("ctx.fk20", c->fk20_ws, bytes);
        c->fk20_cap = bytes;
    }
    *ws = c->fk20_ws;
    return ZKP_OK;
}
int g1ntt_tables(zkp_ctx* c, unsigned log2_n, const uint32_t** domain, const uint64_t** split, unsigned* table_log2, hipStream_t s) {
    if (int rc = kzg_domain(c, log2_n, domain, table_log2, s)) return rc;
    if (c->g1ntt_split_log2 != (int)*table_log2) {
        if (c->g1ntt_split) { HIPCHK(c, hipFree(c->g1ntt_split)); c->g1ntt_split = nullptr; c->g1ntt_split_log2 = -1; }
        HIPCHK(c, hipMalloc((void**)&c->g1ntt_split, zkp::fk20::split_table_bytes(*table_log2)));
        zkp_dbg_alloc("ctx.g1ntt_split", c->g1ntt_split, zkp::fk20::split_table_bytes(*table_log2));
        const hipError_t e = zkp::g1ntt_split_build(*domain, *table_log2, c->g1ntt_split, s);
        if (e != hipSuccess) { (void)hipFree(c->g1ntt_split); c->g1ntt_split = nullptr; }
        HIPCHK(c, e);
        c->g1ntt_split_log2 = (int)*table_log2;
    }
    *split = c->g1ntt_split;
    return ZKP_OK;
}
int grow_bls(zkp_ctx* c, size_t bytes, void** ws) {
    if (bytes > c->bls_cap) {
        if (c->bls_ws) { HIPCHK(c, hipFree(c->bls_ws)); c->bls_ws = nullptr; c->bls_cap = 0; }
        HIPCHK(c, hipMalloc(&c->bls_ws, bytes));
        zkp_dbg_alloc("ctx.bls", c->bls_ws, bytes);
        c->bls_cap = bytes;
    }
    *ws = c->bls_ws;
    return ZKP_OK;
}
int grow_agg(zkp_ctx* c, size_t bytes, void** ws) {
    if (bytes > c->agg_cap) {
        if (c->agg_ws) { HIPCHK(c, hipFree(c->agg_ws)); c->agg_ws = nullptr; c->agg_cap = 0; }
        HIPCHK(c, hipMalloc(&c->agg_ws, bytes));
        zkp_dbg_alloc("ctx.agg", c->agg_ws, bytes);
        c->agg_cap = bytes;
    }
    *ws = c->agg_ws;
    return ZKP_OK;
}
int grow_grp(zkp_ctx* c, size_t bytes, void** ws) {
    if (bytes > c->grp_cap) {
        if (c->grp_ws) { HIPCHK(c, hipFree(c->grp_ws)); c->grp_ws = nullptr; c->grp_cap = 0; }
        HIPCHK(c, hipMalloc(&c->grp_ws, bytes));
        zkp_dbg_alloc("ctx.grp", c->grp_ws, bytes);
        c->grp_cap = bytes;
    }
    *ws = c->grp_ws;
    return ZKP_OK;
}
int grow_minsig(zkp_ctx* c, size_t bytes, void** ws) {
    if (bytes > c->minsig_cap) {
        if (c->minsig_ws) { HIPCHK(c, hipFree(c->minsig_ws)); c->minsig_ws = nullptr; c->minsig_cap = 0; }
        HIPCHK(c, hipMalloc(&c->minsig_ws, bytes));
        zkp_dbg_alloc("ctx.minsig", c->minsig_ws, bytes);
        c->minsig_cap = bytes;
    }
    *ws = c->minsig_ws;
    return ZKP_OK;
}
int grow_prod(zkp_ctx* c, size_t records) { return ensure_prod(c, records); }
int* bls_bad_word(zkp_ctx* c) { return c->validate ? c->d_flag + 2 : nullptr; }
int* validation_word(zkp_ctx* c) { return c->d_flag + 2; }
int mul(zkp_ctx* c, int which, const void* base, size_t stride, const void* sc, size_t n, void* out, void* out_inf, hipStream_t s) {
    return mul_dev(c, which, base, stride, sc, n, out, out_inf, s);
}
int add(zkp_ctx* c, int which, const void* a, const void* inf_a, const void* b, const void* inf_b, size_t n, void* out, void* out_inf, hipStream_t s) {
    return add_dev(c, which, a, inf_a, b, inf_b, n, out, out_inf, s);
}
int grow_msm(zkp_ctx* c, size_t bytes) { return msm_grow(c, bytes); }
int msm(zkp_ctx* c, int which, const void* pts, const void* inf, const void* sc, size_t m, size_t n_msm, void* out, void* out_inf, hipStream_t s) {
    return msm_dev(c, which, pts, inf, sc, m, n_msm, 0, out, out_inf, s, nullptr);
}
int msm_shared(zkp_ctx* c, int which, const void* pts, const void* inf, const void* sc, size_t m, size_t n_msm, void* out, void* out_inf, hipStream_t s) {
    return msm_dev(c, which, pts, inf, sc, m, n_msm, 1, out, out_inf, s, nullptr);
}
int valid(zkp_ctx* c, int which, const void* pts, const void* inf, size_t n, void* status, hipStream_t s) { return valid_dev(c, which, pts, inf, n, status, s); }
int miller_product(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* i1, const uint8_t* i2, size_t n, uint64_t* out, hipStream_t s) {
    return miller_product_dev(c, g1, g2, i1, i2, n, out, s);
}
int gt_is_one(zkp_ctx* c, uint64_t* f, size_t n, uint64_t* gt, int* is_one, hipStream_t s) {
    int rc;
    if ((rc = fp12_product_inplace(c, f, n, s)) || (rc = final_exp_dev(c, f, 1, gt, s))) return rc;
    hipLaunchKernelGGL(k_gt_is_one, dim3(1), dim3(64), 0, s, gt, is_one);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}
}  // namespace ctxop
}  // namespace zkp

extern "C" {

int zkp_g1_mul_endo_batch(zkp_ctx* c, const uint64_t* base, const uint8_t* inf, const uint64_t* ab, size_t n, uint64_t* out, uint8_t* out_inf) {
    if (!c || too_many(n) || (n && (!base || !ab || !out))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const uint64_t* db = (const uint64_t*)io.in(0, base, n * 96);
    const void* dab = io.in(1, ab, n * 16);
    void* dout = io.out(4, out, n * 96);
    void* dinf = io.out(6, out_inf, n);
    const void* di = io.in(2, inf, n);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, db, n * 2)) || (rc = endo_dev(c, db, di, dab, n, dout, dinf, c->stream))) return rc;
    return io.finish();
}
// the batch's thirteen arrays one after the other in slot 0 (256-byte aligned), then the same driver as the _dev flavour
int zkp_pairing_check_batch_rlc(zkp_ctx* c, const zkp_rlc_batch* b, const uint64_t* rand, int flags, int* all_ok) {
    if (rlc_args_bad(c, b, rand, flags, all_ok)) return ZKP_ERR_ARG;
    if (!b->n_checks) { *all_ok = 1; return ZKP_OK; }
    const size_t n = b->n_checks, np = n * b->k, t2 = n * b->s2, t1 = n * b->s1;
    zkp_rlc_batch d = *b;
    const void* drand = rand;
    const void** field[13] = {&d.g1, &d.g2, &d.inf1, &d.inf2, &d.col_g1, &d.col_inf1, &d.fixed_g2, &d.fixed_inf2, &d.col_g2, &d.col_inf2, &d.fixed_g1,
                              &d.fixed_inf1, &drand};
    const size_t bytes[13] = {np * 96, np * 192, np, np, t2 * 96, t2, b->s2 * 192, b->s2, t1 * 192, t1, b->s1 * 96, b->s1, n * 16};
    size_t off[13], total = 0;
    for (int i = 0; i < 13; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    char* dev = (char*)io.slot(0, total);
    for (int i = 0; i < 13; i++) *field[i] = bytes[i] ? io.put(dev + off[i], *field[i], bytes[i]) : nullptr;
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = rlc_validate(&d, [&](const void* p, size_t n_fp) { return validate_dev(c, (const uint64_t*)p, n_fp); })) ||
        (rc = zkp::rlc_check_dev(c, &d, (const uint64_t*)drand, flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

// both point codecs, host pointers (only the compressed flavours cap n): slot 0 the input, slot 4 the output, slot 2 the infinity
// flags (written by a decode, read by an encode), slot 6 the status bytes of a decode
static int codec_host(zkp_ctx* c, bool compressed, bool decode, int which, const void* in, const uint8_t* inf_in, size_t n, void* out,
                      uint8_t* out_inf, uint8_t* status) {
    if (!c || (compressed && too_many(n)) || (n && (!in || !out)) || (decode && n && (!out_inf || !status))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const size_t nw = n * 96 * which, nb = compressed ? nw / 2 : nw;   // wire-point bytes, encoded bytes
    const void* din = io.in(0, in, decode ? nb : nw);
    void* dout = io.out(4, out, decode ? nw : nb);
    void* dinf = decode ? io.out(2, out_inf, n) : (void*)io.in(2, inf_in, n);
    void* dst = io.out(6, status, n);
    int rc;
    if ((rc = io.status()) || (rc = codec_dev(c, compressed, decode, which, din, dinf, n, dout, dinf, dst, c->stream))) return rc;
    return io.finish();
}
int zkp_g1_decode_batch(zkp_ctx* c, const uint8_t* bytes, size_t n, uint64_t* out, uint8_t* out_inf, uint8_t* status) {
    return codec_host(c, false, true, 1, bytes, nullptr, n, out, out_inf, status);
}
int zkp_g2_decode_batch(zkp_ctx* c, const uint8_t* bytes, size_t n, uint64_t* out, uint8_t* out_inf, uint8_t* status) {
    return codec_host(c, false, true, 2, bytes, nullptr, n, out, out_inf, status);
}
int zkp_g1_encode_batch(zkp_ctx* c, const uint64_t* g1, const uint8_t* inf, size_t n, uint8_t* out) {
    return codec_host(c, false, false, 1, g1, inf, n, out, nullptr, nullptr);
}
int zkp_g2_encode_batch(zkp_ctx* c, const uint64_t* g2, const uint8_t* inf, size_t n, uint8_t* out) {
    return codec_host(c, false, false, 2, g2, inf, n, out, nullptr, nullptr);
}
int zkp_g1_decompress_batch(zkp_ctx* c, const uint8_t* bytes, size_t n, uint64_t* out_g1, uint8_t* out_inf, uint8_t* status) {
    return codec_host(c, true, true, 1, bytes, nullptr, n, out_g1, out_inf, status);
}
int zkp_g2_decompress_batch(zkp_ctx* c, const uint8_t* bytes, size_t n, uint64_t* out_g2, uint8_t* out_inf, uint8_t* status) {
    return codec_host(c, true, true, 2, bytes, nullptr, n, out_g2, out_inf, status);
}
int zkp_g1_compress_batch(zkp_ctx* c, const uint64_t* g1, const uint8_t* inf, size_t n, uint8_t* out_bytes) {
    return codec_host(c, true, false, 1, g1, inf, n, out_bytes, nullptr, nullptr);
}
int zkp_g2_compress_batch(zkp_ctx* c, const uint64_t* g2, const uint8_t* inf, size_t n, uint8_t* out_bytes) {
    return codec_host(c, true, false, 2, g2, inf, n, out_bytes, nullptr, nullptr);
}

// both byte strings go to one buffer (PC_BYTES); points_check_dev grows the status / ok slots it writes
static int points_check_host(zkp_ctx* c, const uint8_t* g1_bytes, const uint8_t* g2_bytes, size_t n_checks, size_t k, uint8_t* st1, uint8_t* st2,
                             uint8_t* ok, int* all_ok, bool compressed) {
    if (!c || too_many(n_checks, k) || (n_checks && k && (!g1_bytes || !g2_bytes))) return ZKP_ERR_ARG;
    if (all_ok) *all_ok = 1;
    if (!n_checks) return ZKP_OK;
    HostIO io(c);
    const size_t np = n_checks * k;
    const size_t sz1 = compressed ? 48 : 96, sz2 = 2 * sz1;
    int rc;
    if ((rc = io.status()) || (rc = ensure_pc(c, PC_BYTES, np * (sz1 + sz2) + 8))) return rc;
    uint8_t* d1 = (uint8_t*)c->pc[PC_BYTES];
    uint8_t* d2 = d1 + np * sz1;
    io.put(d1, g1_bytes, np * sz1);
    io.put(d2, g2_bytes, np * sz2);
    if ((rc = io.status()) || (rc = points_check_dev(c, d1, d2, n_checks, k, nullptr, nullptr, nullptr, c->d_flag + 1, c->stream, compressed))) return rc;
    io.get(st1, c->pc[PC_ST1], np);
    io.get(st2, c->pc[PC_ST2], np);
    io.get(ok, c->pc[PC_OK], n_checks);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    return io.finish();
}
int zkp_points_check_batch(zkp_ctx* c, const uint8_t* g1_bytes, const uint8_t* g2_bytes, size_t n_checks, size_t k, uint8_t* st1, uint8_t* st2,
                           uint8_t* ok, int* all_ok) {
    return points_check_host(c, g1_bytes, g2_bytes, n_checks, k, st1, st2, ok, all_ok, false);
}
int zkp_points_check_compressed_batch(zkp_ctx* c, const uint8_t* g1_bytes, const uint8_t* g2_bytes, size_t n_checks, size_t k, uint8_t* st1,
                                      uint8_t* st2, uint8_t* ok, int* all_ok) {
    return points_check_host(c, g1_bytes, g2_bytes, n_checks, k, st1, st2, ok, all_ok, true);
}

// square-root hooks (host pointers, like zkp_fp_op_batch): which = 1 Fp::sqrt, 2 Fp2::sqrt
static int sqrt_host(zkp_ctx* c, int which, const uint64_t* a, size_t n, uint64_t* out, uint8_t* is_square) {
    if (!c || n > 0x7fffffffu || (n && (!a || !out || !is_square))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const size_t bytes = n * 48 * which;
    const uint64_t* da = (const uint64_t*)io.in(0, a, bytes);
    void* dout = io.out(4, out, bytes);
    void* dsq = io.out(6, is_square, n);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, da, n * which)) ||
        (rc = coop_rc(c, "sqrt", zkp_cmp::sqrt_ref(which, da, n, (uint64_t*)dout, (uint8_t*)dsq, c->stream))))
        return rc;
    return io.finish();
}
int zkp_fp_sqrt_batch(zkp_ctx* c, const uint64_t* a, size_t n, uint64_t* out, uint8_t* is_square) { return sqrt_host(c, 1, a, n, out, is_square); }
int zkp_fp2_sqrt_batch(zkp_ctx* c, const uint64_t* a, size_t n, uint64_t* out, uint8_t* is_square) { return sqrt_host(c, 2, a, n, out, is_square); }

int zkp_fp_op_batch(zkp_ctx* c, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    const int base = op & ~ZKP_FP_CORE28;
    const bool unary = base == ZKP_FP_NEG || base == ZKP_FP_SQUARE || base == ZKP_FP_INVERT;
    if (!c || op < 0 || base > ZKP_FP_INVERT || n > 0x7fffffffu || (n && (!a || !out || (!unary && !b)))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const uint64_t* da = (const uint64_t*)io.in(0, a, n * 48);
    uint64_t* db = (uint64_t*)io.slot(1, n * 48);   // the kernels take it whether or not the operation reads it
    io.put(db, unary ? nullptr : b, n * 48);
    uint64_t* dout = (uint64_t*)io.out(4, out, n * 48);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, da, n)) || (!unary && (rc = validate_dev(c, db, n)))) return rc;
    if (op & ZKP_FP_CORE28) {   // the 14 x 28-bit carry-free core of the cooperative family
        HIPCHK(c, zkp::coop_fp28_op(base, da, db, n, dout, c->stream));
    } else {
        hipLaunchKernelGGL(k_fp_op, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, base, da, (const uint64_t*)db, n, dout);
        HIPCHK(c, hipGetLastError());
    }
    return io.finish();
}

int zkp_tower_op_batch(zkp_ctx* c, int op, const uint64_t* a, const uint64_t* b, size_t n, uint32_t repeat, uint64_t* out) {
    const bool binary = op == ZKP_TOWER_FP2_MUL || op == ZKP_TOWER_FP6_MUL || op == ZKP_TOWER_FP12_MUL || op == ZKP_TOWER_FP12_MUL_BY_014 ||
                        op == ZKP_TOWER_FP2_MUL_FP || op == ZKP_TOWER_FP6_MUL_BY_1 || op == ZKP_TOWER_FP6_MUL_BY_01;
    if (!c || op < 0 || op > ZKP_TOWER_FP12_INVERT || n > 0x3fffffffu || (n && (!a || !out || (binary && !b)))) return ZKP_ERR_ARG;
    if (op == ZKP_TOWER_FP12_CYCLOTOMIC_DECOMPRESS && !zkp::coop_selected(&c->coop, c->kernel)) return ZKP_ERR_ARG;
    if (op == ZKP_TOWER_FP12_CYCLOTOMIC_POW2K && (repeat < 1 || repeat > 64)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    // one buffer: the a records, then the b records (the step programs read record check + n as their second operand)
    uint64_t* d_a = (uint64_t*)io.slot(5, 2 * n * 576);
    uint64_t* dout = (uint64_t*)io.out(4, out, n * 576);
    int rc;
    if ((rc = io.status())) return rc;
    uint64_t* d_b = d_a + 72 * n;
    io.put(d_a, a, n * 576);
    io.put(d_b, binary ? b : nullptr, n * 576);
    if ((rc = io.status()) || (rc = validate_dev(c, d_a, (binary ? 2 : 1) * n * 12))) return rc;
    if (zkp::coop_selected(&c->coop, c->kernel)) {
        const hipError_t e = zkp::coop_tower_op(&c->coop, op, d_a, n, repeat, dout, c->stream);
        if (e != hipSuccess) { c->err = std::string("coop_tower_op: ") + hipGetErrorString(e); return ZKP_ERR_HIP; }
    } else {
        hipLaunchKernelGGL(k_tower_op, dim3(grid_for(n, TPB)), dim3(TPB), 0, c->stream, op, d_a, binary ? d_b : nullptr, n, repeat, dout);
        HIPCHK(c, hipGetLastError());
    }
    return io.finish();
}

// ---------------------------------------------------------------- several GPUs behind one call
// one host thread drives n_ctx contexts (normally one per GPU of the node; several on one GPU work
// too), every context takes a contiguous block of the checks - a check's k pairs and its shared final exponentiation
// stay on one GPU - uploads it on its own stream, runs the same pipeline as zkp_pairing_check_batch / zkp_pairing_batch,
// and downloads its results; the per-context AND flags are combined on the host.  Nothing crosses xGMI: the data path
// has no collective.  (The one-process-per-GPU form of the same call is zkp_pairing_check_batch per rank plus ONE
// ncclAllReduce(count = 1, ncclInt32, ncclMin) of the flag - RCCL has no bitwise AND; INTEGRATION.md.)
static int multi_impl(zkp_ctx* const* ctxs, int n_ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2,
                      size_t n_checks, size_t k, uint64_t* out_gt, uint8_t* ok, int* all_ok) {
    if (!ctxs || n_ctx <= 0 || n_ctx > 64 || too_many(n_checks, k) || (n_checks && k && (!g1 || !g2))) return ZKP_ERR_ARG;
    for (int j = 0; j < n_ctx; j++) {
        if (!ctxs[j]) return ZKP_ERR_ARG;
        for (int i = 0; i < j; i++)
            if (ctxs[i] == ctxs[j]) return ZKP_ERR_ARG;
    }
    if (all_ok) *all_ok = 1;
    if (!n_checks) return ZKP_OK;
    int flags[64];
    int rc = ZKP_OK, used = 0;
    const size_t base = n_checks / n_ctx, rem = n_checks % n_ctx;
    // workspace of every context first: an allocation synchronises its device, and must not do so between another context's
    // upload and launch.  After this pass the loop below only queues work: from page-locked arrays (zkp_host_alloc /
    // zkp_host_register) no context's start waits for another context's copy.
    for (int j = 0; j < n_ctx; j++) {
        zkp_ctx* c = ctxs[j];
        const size_t m = base + ((size_t)j < rem ? 1 : 0);
        if (!m) continue;
        if ((rc = bind(c))) return rc;
        if ((rc = ensure(c, 0, m * k * 96)) || (rc = ensure(c, 1, m * k * 192)) || (inf1 && (rc = ensure(c, 2, m * k))) ||
            (inf2 && (rc = ensure(c, 3, m * k))) || (out_gt && (rc = ensure(c, 4, m * 576))) || (rc = ensure(c, 6, m)))
            return rc;
    }
    for (int j = 0; j < n_ctx && rc == ZKP_OK; j++) {
        zkp_ctx* c = ctxs[j];
        const size_t lo = j * base + ((size_t)j < rem ? j : rem), m = base + ((size_t)j < rem ? 1 : 0), p0 = lo * k;
        flags[j] = 1;
        used = j + 1;
        if (!m) continue;
        if ((rc = bind(c))) break;
        if (c->ws_busy) (void)hipStreamWaitEvent(c->stream, c->ws_busy, 0);
        Staging io(c);   // not a HostIO: the contexts are drained together below
        Staged st = {nullptr, nullptr, nullptr, nullptr};
        if (k && (rc = stage_pairs(io, g1 + 12 * p0, g2 + 24 * p0, inf1 ? inf1 + p0 : nullptr, inf2 ? inf2 + p0 : nullptr, m * k, &st))) break;
        void* dgt = out_gt ? io.out(4, out_gt + 72 * lo, m * 576) : nullptr;
        void* dok = io.out(6, ok ? ok + lo : nullptr, m);
        io.get(&flags[j], c->d_flag + 1, sizeof(int));
        if ((rc = io.status()) || (rc = pairing_dev(c, st.g1, st.g2, st.i1, st.i2, m, k, (uint64_t*)dgt, (uint8_t*)dok, c->d_flag + 1, c->stream)) ||
            (rc = io.send()))
            break;
        if (hipEventRecord(c->ws_busy, c->stream) != hipSuccess) { c->err = "zkp_pairing_*_multi: hipEventRecord failed"; rc = ZKP_ERR_HIP; }
    }
    // whatever happened, nothing may still be copying from or into the caller's arrays when the call returns
    for (int j = 0; j < used; j++) {
        zkp_ctx* c = ctxs[j];
        if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
            if (rc == ZKP_OK) { c->err = "zkp_pairing_*_multi: stream synchronisation failed"; rc = ZKP_ERR_HIP; }
        }
    }
    if (rc != ZKP_OK) return rc;
    int all = 1;
    for (int j = 0; j < used; j++) all &= flags[j] ? 1 : 0;
    if (all_ok) *all_ok = all;
    return ZKP_OK;
}
int zkp_pairing_check_batch_multi(zkp_ctx* const* ctxs, int n_ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2,
                                  size_t n_checks, size_t k, uint8_t* ok, int* all_ok) {
    return multi_impl(ctxs, n_ctx, g1, g2, inf1, inf2, n_checks, k, nullptr, ok, all_ok);
}
int zkp_pairing_batch_multi(zkp_ctx* const* ctxs, int n_ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n,
                            uint64_t* out_gt, uint8_t* ok, int* all_ok) {
    if (n && !out_gt) return ZKP_ERR_ARG;
    return multi_impl(ctxs, n_ctx, g1, g2, inf1, inf2, n, 1, out_gt, ok, all_ok);
}

// ---------------------------------------------------------------- one rank per GPU: the RCCL collective behind the ABI
#define NCCLCHK(ctx, call)                                                                      \
    do {                                                                                        \
        ncclResult_t r__ = (call);                                                              \
        if (r__ != ncclSuccess) {                                                               \
            (ctx)->err = std::string(#call) + ": " + ncclGetErrorString(r__);                   \
            return ZKP_ERR_COMM;                                                                \
        }                                                                                       \
    } while (0)
static_assert(ZKP_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "the header's id size is RCCL's");

int zkp_comm_unique_id(void* out_id) {
    if (!out_id) return ZKP_ERR_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return ZKP_ERR_COMM;
    memcpy(out_id, id.internal, NCCL_UNIQUE_ID_BYTES);
    return ZKP_OK;
}
int zkp_comm_init_rank(zkp_ctx* c, int nranks, int rank, const void* unique_id) {
    if (!c || !unique_id || nranks < 1 || rank < 0 || rank >= nranks) return ZKP_ERR_ARG;
    if (c->comm) { c->err = "the context already has a communicator"; return ZKP_ERR_ARG; }
    int rc = bind(c);
    if (rc) return rc;
    ncclUniqueId id;
    memcpy(id.internal, unique_id, NCCL_UNIQUE_ID_BYTES);
    // EVERY rank enters the bootstrap first (round 6): ncclCommInitRank blocks until all nranks ranks have called it, so a rank that
    // returned on a local failure BEFORE it - round 5 allocated the all-gather records first - left its peers waiting for ever.  The
    // records are allocated behind it; a rank that cannot have them aborts its communicator and returns ZKP_ERR_OOM.  Its peers hold a
    // communicator with a member that is gone and cannot know: a failed zkp_comm_init_rank MUST be told to the other ranks by the
    // host's own means (bench.py: one gloo all-reduce of the status) BEFORE anyone enters a collective - include/zkp_pairings.h.
    ncclResult_t r = ncclCommInitRank(&c->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        c->comm = nullptr;
        c->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r);
        return ZKP_ERR_COMM;
    }
    if (hipMalloc((void**)&c->comm_buf, ((size_t)nranks + 3) * 576) != hipSuccess) {
        (void)hipGetLastError();
        (void)ncclCommAbort(c->comm);        // needs no peer (ncclCommDestroy may wait for them)
        c->comm = nullptr;
        c->comm_buf = nullptr;
        c->err = "zkp_comm_init_rank: no memory for the communicator's Fp12 records";
        return ZKP_ERR_OOM;
    }
    c->comm_nranks = nranks;
    c->comm_rank = rank;
    return ZKP_OK;
}
int zkp_comm_destroy(zkp_ctx* c) {
    if (!c) return ZKP_ERR_ARG;
    if (!c->comm) return ZKP_OK;
    int rc = bind(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ncclComm_t comm = c->comm;
    c->comm = nullptr;
    c->comm_nranks = c->comm_rank = 0;
    if (c->comm_buf) { (void)hipFree(c->comm_buf); c->comm_buf = nullptr; }
    NCCLCHK(c, ncclCommDestroy(comm));
    return ZKP_OK;
}
int zkp_comm_info(const zkp_ctx* c, int* nranks, int* rank) {
    if (!c) return ZKP_ERR_ARG;
    if (nranks) *nranks = c->comm ? c->comm_nranks : 0;
    if (rank) *rank = c->comm ? c->comm_rank : 0;
    return ZKP_OK;
}
// AND of {0,1} flags = MIN (RCCL has no bitwise AND): ONE ncclAllReduce(count = 1, ncclInt32, ncclMin), in place
static int and_allreduce(zkp_ctx* c, int* d_flag, hipStream_t s) {
    if (!c->comm) { c->err = "no communicator: call zkp_comm_init_rank first"; return ZKP_ERR_COMM; }
    NCCLCHK(c, ncclAllReduce(d_flag, d_flag, 1, ncclInt32, ncclMin, c->comm, s));
    return ZKP_OK;
}
// the collective of the resident flavours after the rank's own work: a local failure turns the rank's flag into 0 and still joins
static int reduce_after_local(zkp_ctx* c, int rc_local, int* d_all_ok, hipStream_t s) {
    if (rc_local) {
        const std::string first = c->err;
        if (bind(c) != ZKP_OK || hipMemsetAsync(d_all_ok, 0, sizeof(int), s) != hipSuccess) return rc_local;      // nothing left to join with
        (void)and_allreduce(c, d_all_ok, s);
        c->err = first;
        return rc_local;
    }
    return and_allreduce(c, d_all_ok, s);
}
// ... and of the host-pointer flavours: the rank's local AND (0 when its own call failed) goes to the device, through the collective
// and back; the rank's own status is what the call returns
static int host_flag_allreduce(zkp_ctx* c, int rc_local, int local, int* all_ok) {
    if (rc_local) local = 0;
    const std::string first = c->err;
    HostIO io(c);
    int rc = io.status();
    if (rc) return rc_local ? rc_local : rc;
    // the flag reaches the device by a kernel argument, not by a copy that could fail before the collective: whatever happened locally,
    // this rank enters the all-reduce its peers are waiting in
    hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, c->stream, c->d_flag + 1, local ? 1 : 0);
    if (hipGetLastError() != hipSuccess && hipMemsetAsync(c->d_flag + 1, 0, sizeof(int), c->stream) != hipSuccess) {
        if (!rc_local) { c->err = "the AND flag could not be written to the device"; return ZKP_ERR_HIP; }
        return rc_local;      // nothing left to join with
    }
    if ((rc = and_allreduce(c, c->d_flag + 1, c->stream))) return rc_local ? rc_local : rc;
    int all = 0;
    HIPCHK(c, hipMemcpyAsync(&all, c->d_flag + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *all_ok = all;
    if (rc_local) c->err = first;
    return rc_local;
}
int zkp_and_allreduce_dev(zkp_ctx* c, void* d_flag, void* stream) {
    if (!c || !d_flag) return ZKP_ERR_ARG;
    int rc = bind(c);
    if (rc) return rc;
    return and_allreduce(c, (int*)d_flag, S(stream));
}
int zkp_pairing_check_batch_allreduce_dev(zkp_ctx* c, const void* g1, const void* g2, const void* i1, const void* i2, size_t n_checks, size_t k,
                                          void* ok, void* all_ok, void* stream) {
    if (!c || !all_ok) return ZKP_ERR_ARG;
    if (!c->comm) { c->err = "no communicator: call zkp_comm_init_rank first"; return ZKP_ERR_COMM; }
    // a rank with an empty block still sets its flag to 1; a rank whose own block FAILED still takes part, with flag 0, so that no
    // peer hangs in the collective (every rank then reads 0; this rank returns its own error)
    const int rc_local = zkp_pairing_check_batch_dev(c, g1, g2, i1, i2, n_checks, k, ok, all_ok, stream);
    return reduce_after_local(c, rc_local, (int*)all_ok, S(stream));
}
int zkp_pairing_gt_check_batch_allreduce_dev(zkp_ctx* c, const void* g1, const void* g2, const void* i1, const void* i2, size_t n_checks, size_t k,
                                             void* out_gt, void* ok, void* all_ok, void* stream) {
    if (!c || !all_ok) return ZKP_ERR_ARG;
    if (!c->comm) { c->err = "no communicator: call zkp_comm_init_rank first"; return ZKP_ERR_COMM; }
    const int rc_local = zkp_pairing_gt_check_batch_dev(c, g1, g2, i1, i2, n_checks, k, out_gt, ok, all_ok, stream);
    return reduce_after_local(c, rc_local, (int*)all_ok, S(stream));
}
int zkp_pairing_check_batch_allreduce(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n_checks,
                                      size_t k, uint8_t* ok, int* all_ok) {
    if (!c || !all_ok) return ZKP_ERR_ARG;
    if (!c->comm) { c->err = "no communicator: call zkp_comm_init_rank first"; return ZKP_ERR_COMM; }
    // the rank's own block through the host-pointer entry point (uploads, kernels, downloads; it leaves the local AND in *all_ok),
    // then the flag goes back to the device for the collective: every rank calls this exactly once per global check, whatever
    // its own block's size or status - a rank that failed locally still takes part (with flag 0) so that no peer hangs
    int local = 1;
    const int rc_local = zkp_pairing_check_batch(c, g1, g2, inf1, inf2, n_checks, k, ok, &local);
    return host_flag_allreduce(c, rc_local, local, all_ok);
}
int zkp_points_check_batch_allreduce_dev(zkp_ctx* c, const void* b1, const void* b2, size_t n_checks, size_t k, void* st1, void* st2, void* ok,
                                         void* all_ok, void* stream) {
    if (!c || !all_ok) return ZKP_ERR_ARG;
    if (!c->comm) { c->err = "no communicator: call zkp_comm_init_rank first"; return ZKP_ERR_COMM; }
    const int rc_local = zkp_points_check_batch_dev(c, b1, b2, n_checks, k, st1, st2, ok, all_ok, stream);
    return reduce_after_local(c, rc_local, (int*)all_ok, S(stream));
}
int zkp_points_check_batch_allreduce(zkp_ctx* c, const uint8_t* b1, const uint8_t* b2, size_t n_checks, size_t k, uint8_t* st1, uint8_t* st2,
                                     uint8_t* ok, int* all_ok) {
    if (!c || !all_ok) return ZKP_ERR_ARG;
    if (!c->comm) { c->err = "no communicator: call zkp_comm_init_rank first"; return ZKP_ERR_COMM; }
    int local = 1;
    const int rc_local = zkp_points_check_batch(c, b1, b2, n_checks, k, st1, st2, ok, &local);
    return host_flag_allreduce(c, rc_local, local, all_ok);
}
int zkp_pairing_product_check_allgather(zkp_ctx* c, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2, size_t n,
                                        uint64_t* out_gt, int* is_one) {
    if (!c) return ZKP_ERR_ARG;
    if (!c->comm) { c->err = "no communicator: call zkp_comm_init_rank first"; return ZKP_ERR_COMM; }
    const bool bad_args = (n && (!g1 || !g2)) || n > 0x7fffffffu;
    if (bad_args) { n = 0; c->err = "zkp_pairing_product_check_allgather: null points / too many pairs"; }
    HostIO io(c);
    int rc = io.status();
    if (rc) return rc;
    const size_t R = (size_t)c->comm_nranks;
    // this rank's Miller product -> the communicator's record 0 (the identity for an empty block), gathered into records 1..R.  A rank
    // whose own part fails - bad arguments, staging, an allocation that runs out of memory, a launch error - still joins the collective,
    // with the ZERO record, so that the product is 0 and every rank reads is_one = 0 (no peer hangs, none passes a check this rank's
    // pairs never entered), and returns its own error afterwards.  The records the collective itself needs belong to the communicator
    // (zkp_comm_init_rank allocated them): nothing that can fail stands between this point and ncclAllGather.
    uint64_t* const mine = c->comm_buf;
    uint64_t* const gathered = c->comm_buf + 72;
    uint64_t* const total = c->comm_buf + 72 * (R + 1);
    uint64_t* const gt = c->comm_buf + 72 * (R + 2);
    Staged st = {nullptr, nullptr, nullptr, nullptr};
    int rc_local = bad_args ? ZKP_ERR_ARG : ZKP_OK;
    if (!rc_local && n) rc_local = stage_pairs(io, g1, g2, inf1, inf2, n, &st);
    if (!rc_local) rc_local = miller_product_dev(c, st.g1, st.g2, st.i1, st.i2, n, mine, c->stream);
    const std::string first = c->err;
    if (rc_local) {
        if (bind(c) != ZKP_OK || hipMemsetAsync(mine, 0, 576, c->stream) != hipSuccess) return rc_local;
    }
    NCCLCHK(c, ncclAllGather(mine, gathered, 72, ncclUint64, c->comm, c->stream));
    if ((rc = fp12_product_dev(c, gathered, R, total, c->stream))) return rc_local ? rc_local : rc;
    if ((rc = final_exp_dev(c, total, 1, gt, c->stream))) return rc_local ? rc_local : rc;
    hipLaunchKernelGGL(k_gt_is_one, dim3(1), dim3(64), 0, c->stream, (const uint64_t*)gt, c->d_flag);
    HIPCHK(c, hipGetLastError());
    int one = 0;
    if (out_gt) HIPCHK(c, hipMemcpyAsync(out_gt, gt, 576, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&one, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (is_one) *is_one = one;
    if (rc_local) c->err = first;
    return rc_local;
}

// page-locked host memory for the host-pointer entry points (header: "pinned host memory")
int zkp_host_alloc(size_t bytes, void** out_ptr) {
    if (!out_ptr || !bytes) return ZKP_ERR_ARG;
    *out_ptr = nullptr;
    const bool ok = hipHostMalloc(out_ptr, bytes, hipHostMallocPortable) == hipSuccess;
    if (ok) zkp_dbg_alloc("host_alloc", *out_ptr, bytes);
    return ok ? ZKP_OK : ZKP_ERR_HIP;
}
int zkp_host_free(void* ptr) {
    if (ptr) zkp_dbg_alloc("host_free", ptr, 0);
    return !ptr || hipHostFree(ptr) == hipSuccess ? ZKP_OK : ZKP_ERR_HIP;
}
int zkp_host_register(void* ptr, size_t bytes) {
    if (!ptr || !bytes) return ZKP_ERR_ARG;
    // whole pages of its own only (header: pinned host memory): registrations that share a page corrupt the runtime's bookkeeping
    static const long page = sysconf(_SC_PAGESIZE) > 0 ? sysconf(_SC_PAGESIZE) : 4096;
    if (((uintptr_t)ptr | bytes) & (uintptr_t)(page - 1)) return ZKP_ERR_ARG;
    zkp_dbg_alloc("host_register", ptr, bytes);
    return hipHostRegister(ptr, bytes, hipHostRegisterPortable) == hipSuccess ? ZKP_OK : ZKP_ERR_HIP;
}
int zkp_host_unregister(void* ptr) {
    if (!ptr) return ZKP_ERR_ARG;
    zkp_dbg_alloc("host_unregister", ptr, 0);
    return hipHostUnregister(ptr) == hipSuccess ? ZKP_OK : ZKP_ERR_HIP;
}

// measurement helper: a one-wavefront clock probe on `stream` (asynchronous); d_out receives two u64: shader clock ticks
// and wall clock ticks over about spin_us microseconds; *wall_khz (host) is the wall clock's rate.
int zkp_clock_probe_dev(zkp_ctx* c, void* stream, unsigned spin_us, void* d_out, int* wall_khz) {
    if (!c || !d_out || !wall_khz || spin_us == 0 || spin_us > 1000000u) return ZKP_ERR_ARG;
    int rc = bind(c);
    if (rc) return rc;
    int khz = 0;
    HIPCHK(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    if (khz <= 0) { c->err = "wall clock rate unknown"; return ZKP_ERR_HIP; }
    *wall_khz = khz;
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, S(stream), (unsigned long long*)d_out, (unsigned long long)spin_us * (unsigned long long)khz / 1000ull);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
}

int zkp_time_coop_step(zkp_ctx* c, int which, size_t n, float* ms) {
    if (!c || !ms) return ZKP_ERR_ARG;
    HostIO io(c);   // the timing programs reuse the workspace of pipeline 0: wait for *_dev calls queued on other streams, drain on exit
    if (int rc = io.status()) return rc;
    HIPCHK(c, zkp::coop_time_prog(&c->coop, which, n, c->stream, c->ev0, c->ev1, ms));
    return ZKP_OK;
}

int zkp_time_pairing_dev(zkp_ctx* c, const void* g1, const void* g2, size_t n, void* out, int reps, float* avg_ms) {
    if (!c || !g1 || !g2 || !out || reps <= 0 || !avg_ms) return ZKP_ERR_ARG;
    HostIO io(c);   // same workspace discipline as every host-synchronous entry point
    int rc = io.status();
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (int r = 0; r < reps; r++)
        if ((rc = pairing_dev(c, (const uint64_t*)g1, (const uint64_t*)g2, nullptr, nullptr, n, 1, (uint64_t*)out, nullptr, nullptr, c->stream))) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *avg_ms = ms / reps;
    return ZKP_OK;
}


int zkp_profile_pairing_dev(zkp_ctx* c, const void* g1, const void* g2, size_t n, void* out, float* ms, int* launches) {
    if (!c || !g1 || !g2 || !out || !ms || !launches || !n || too_many(n)) return ZKP_ERR_ARG;
    if (!zkp::coop_selected(&c->coop, c->kernel)) { c->err = "zkp_profile_pairing_dev: the cooperative kernel family is not selected"; return ZKP_ERR_ARG; }
    HostIO io(c);
    if (int rc = io.status()) return rc;
    return coop_rc(c, "coop_profile_pairing", zkp::coop_profile_pairing(&c->coop, (const uint64_t*)g1, (const uint64_t*)g2, n, (uint64_t*)out, ms, launches, c->stream));
}

}  // extern "C"

// ---------------------------------------------------------------- Fr, the Fr fold and the batched Groth16 verifier (zkp_groth16.hip)
namespace {
// validation mode for Fr elements: the host flavour reads the word back, the _dev flavour ORs into the sticky one
int validate_fr_dev(zkp_ctx* c, const void* d, size_t n) {
    if (!c->validate || !n || !d) return ZKP_OK;
    HIPCHK(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
    HIPCHK(c, zkp::fr_check_canonical((const uint64_t*)d, n, c->d_flag, c->stream));
    int bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) { c->err = "input limbs >= r"; return ZKP_ERR_NONCANONICAL; }
    return ZKP_OK;
}
int validate_fr_on_stream(zkp_ctx* c, const void* d, size_t n, hipStream_t s) {
    if (!c->validate || !n || !d) return ZKP_OK;
    HIPCHK(c, zkp::fr_check_canonical((const uint64_t*)d, n, c->d_flag + 2, s));
    return ZKP_OK;
}
bool fr_op_unary(int op) { return op == ZKP_FR_NEG || op == ZKP_FR_SQUARE || op == ZKP_FR_INVERT; }
bool fr_op_args_bad(const zkp_ctx* c, int op, const void* a, const void* b, size_t n, const void* out) {
    return !c || op < 0 || op > ZKP_FR_INVERT || n > 0x7fffffffu || (n && (!a || !out || (!fr_op_unary(op) && !b)));
}
// the fold on device pointers: zeros for n == 0, else the partial sums in the context's workspace and the two stages
int fr_fold_dev(zkp_ctx* c, const void* w, const void* x, size_t n, size_t l, void* out, void* sum_w, hipStream_t s) {
    if (!n) {
        if (l) HIPCHK(c, hipMemsetAsync(out, 0, l * 32, s));
        if (sum_w) HIPCHK(c, hipMemsetAsync(sum_w, 0, 32, s));
        return ZKP_OK;
    }
    const zkp::g16::FoldLayout L = zkp::g16::fold_layout(zkp::g16::fold_plan(n, l));
    void* ws = nullptr;
    if (int rc = zkp::ctxop::grow_g16(c, L.total, &ws)) return rc;
    return coop_rc(c, "fr_fold", zkp::fr_fold((char*)ws + L.part, (char*)ws + L.sum, (const uint64_t*)w, (const uint64_t*)x, n, l, (uint64_t*)out,
                                              (uint64_t*)sum_w, nullptr, s));
}
bool fr_fold_args_bad(const zkp_ctx* c, const void* w, const void* x, size_t n, size_t l, const void* out) {
    return !c || zkp::g16::fold_args_bad(n, l) || (l && !out) || (n && (!w || (l && !x)));
}
bool g16_args_bad(const zkp_ctx* c, const zkp_groth16_vk* vk, const zkp_groth16_batch* b, const void* rand, int flags, const void* all_ok) {
    if (!c || !vk || !b || !all_ok || zkp::g16::args_bad(b->n, vk->n_inputs, flags)) return true;
    if (!b->n) return false;
    return !rand || !vk->alpha_g1 || !vk->beta_g2 || !vk->gamma_g2 || !vk->delta_g2 || !vk->ic || !b->a || !b->b || !b->c || (vk->n_inputs && !b->inputs);
}
// validation mode: v(pointer, Fp count) over every coordinate array of the key and the batch
template <class V>
int g16_validate(const zkp_groth16_vk* vk, const zkp_groth16_batch* b, V&& v) {
    int rc;
    if ((rc = v(b->a, b->n * 2)) || (rc = v(b->b, b->n * 4)) || (rc = v(b->c, b->n * 2)) || (rc = v(vk->alpha_g1, 2)) || (rc = v(vk->beta_g2, 4)) ||
        (rc = v(vk->gamma_g2, 4)) || (rc = v(vk->delta_g2, 4)) || (rc = v(vk->ic, (vk->n_inputs + 1) * 2)))
        return rc;
    return ZKP_OK;
}
}  // namespace

extern "C" {

int zkp_fr_op_batch_dev(zkp_ctx* c, int op, const void* a, const void* b, size_t n, void* out, void* stream) {
    if (fr_op_args_bad(c, op, a, b, n, out)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    int rc;
    if ((rc = validate_fr_on_stream(c, a, n, S(stream))) || (!fr_op_unary(op) && (rc = validate_fr_on_stream(c, b, n, S(stream))))) return rc;
    return coop_rc(c, "fr_op", zkp::fr_op(op, (const uint64_t*)a, (const uint64_t*)b, n, (uint64_t*)out, S(stream)));
}
int zkp_fr_op_batch(zkp_ctx* c, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    if (fr_op_args_bad(c, op, a, b, n, out)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    const bool unary = fr_op_unary(op);
    HostIO io(c);
    const void* da = io.in(0, a, n * 32);
    const void* db = unary ? nullptr : io.in(1, b, n * 32);
    void* dout = io.out(4, out, n * 32);
    int rc;
    if ((rc = io.status()) || (rc = validate_fr_dev(c, da, n)) || (rc = validate_fr_dev(c, db, n)) ||
        (rc = coop_rc(c, "fr_op", zkp::fr_op(op, (const uint64_t*)da, (const uint64_t*)db, n, (uint64_t*)dout, c->stream))))
        return rc;
    return io.finish();
}
int zkp_fr_from_wide_batch_dev(zkp_ctx* c, const void* bytes, size_t n, void* out, void* stream) {
    if (!c || n > 0x7fffffffu || (n && (!bytes || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    return coop_rc(c, "fr_from_wide", zkp::fr_from_wide((const uint8_t*)bytes, n, (uint64_t*)out, S(stream)));
}
int zkp_fr_from_wide_batch(zkp_ctx* c, const uint8_t* bytes, size_t n, uint64_t* out) {
    if (!c || n > 0x7fffffffu || (n && (!bytes || !out))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const void* din = io.in(0, bytes, n * 64);
    void* dout = io.out(4, out, n * 32);
    int rc;
    if ((rc = io.status()) || (rc = coop_rc(c, "fr_from_wide", zkp::fr_from_wide((const uint8_t*)din, n, (uint64_t*)dout, c->stream)))) return rc;
    return io.finish();
}
int zkp_fr_fold_batch_dev(zkp_ctx* c, const void* w, const void* x, size_t n, size_t l, void* out, void* sum_w, void* stream) {
    if (fr_fold_args_bad(c, w, x, n, l, out)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int rc;
    if ((rc = validate_fr_on_stream(c, w, n, S(stream))) || (rc = validate_fr_on_stream(c, x, n * l, S(stream)))) return rc;
    return fr_fold_dev(c, w, x, n, l, out, sum_w, S(stream));
}
int zkp_fr_fold_batch(zkp_ctx* c, const uint64_t* w, const uint64_t* x, size_t n, size_t l, uint64_t* out, uint64_t* sum_w) {
    if (fr_fold_args_bad(c, w, x, n, l, out)) return ZKP_ERR_ARG;
    if (!n) {
        if (l) memset(out, 0, l * 32);
        if (sum_w) memset(sum_w, 0, 32);
        return ZKP_OK;
    }
    HostIO io(c);
    const void* dw = io.in(0, w, n * 32);
    const void* dx = l ? io.in(1, x, n * l * 32) : nullptr;
    char* dout = (char*)io.slot(4, (l + 1) * 32);   // the l outputs, then the sum of the weights
    if (dout) {
        io.get(l ? out : nullptr, dout, l * 32);
        io.get(sum_w, dout + l * 32, 32);
    }
    int rc;
    if ((rc = io.status()) || (rc = validate_fr_dev(c, dw, n)) || (rc = validate_fr_dev(c, dx, n * l)) ||
        (rc = fr_fold_dev(c, dw, dx, n, l, dout, sum_w ? dout + l * 32 : nullptr, c->stream)))
        return rc;
    return io.finish();
}
int zkp_groth16_verify_batch_dev(zkp_ctx* c, const zkp_groth16_vk* vk, const zkp_groth16_batch* b, const void* rand, int flags, void* all_ok,
                                 void* stream) {
    if (g16_args_bad(c, vk, b, rand, flags, all_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (b->n)
        if (int rc = g16_validate(vk, b, [&](const void* d, size_t n_fp) { return validate_on_stream(c, d, n_fp, S(stream)); })) return rc;
    return zkp::groth16_check_dev(c, vk, b, (const uint64_t*)rand, flags, (int*)all_ok, S(stream));
}
// the key's and the batch's thirteen arrays one after the other in slot 0 (256-byte aligned), then the same driver as the _dev flavour
int zkp_groth16_verify_batch(zkp_ctx* c, const zkp_groth16_vk* vk, const zkp_groth16_batch* b, const uint64_t* rand, int flags, int* all_ok) {
    if (g16_args_bad(c, vk, b, rand, flags, all_ok)) return ZKP_ERR_ARG;
    if (!b->n) { *all_ok = 1; return ZKP_OK; }
    const size_t n = b->n, l = vk->n_inputs;
    zkp_groth16_vk dv = *vk;
    zkp_groth16_batch d = *b;
    const void* drand = rand;
    const void** field[13] = {&d.a, &d.inf_a, &d.b, &d.inf_b, &d.c, &d.inf_c, &d.inputs, &dv.alpha_g1, &dv.beta_g2, &dv.gamma_g2, &dv.delta_g2, &dv.ic, &drand};
    const size_t bytes[13] = {n * 96, n, n * 192, n, n * 96, n, n * l * 32, 96, 192, 192, 192, (l + 1) * 96, n * 16};
    size_t off[13], total = 0;
    for (int i = 0; i < 13; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    char* dev = (char*)io.slot(0, total);
    for (int i = 0; i < 13; i++) *field[i] = bytes[i] ? io.put(dev + off[i], *field[i], bytes[i]) : nullptr;
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = g16_validate(&dv, &d, [&](const void* p, size_t n_fp) { return validate_dev(c, (const uint64_t*)p, n_fp); })) ||
        (rc = zkp::groth16_check_dev(c, &dv, &d, (const uint64_t*)drand, flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- batched Fr inversion, barycentric evaluation, the KZG verifier (zkp_kzg.hip)
namespace {
int fr_invert_dev(zkp_ctx* c, const void* a, size_t n, void* out, hipStream_t s) {
    void* ws = nullptr;
    if (int rc = zkp::ctxop::grow_kzg(c, zkp::kzg::inv_plan(n).total, &ws)) return rc;
    return coop_rc(c, "fr_invert", zkp::fr_invert(ws, (const uint64_t*)a, n, (uint64_t*)out, s));
}
int fr_eval_dev(zkp_ctx* c, const void* evals, const void* z, size_t n_poly, unsigned log2_n, int flags, void* out, hipStream_t s) {
    void* ws = nullptr;
    const uint32_t* table = nullptr;
    unsigned table_log2 = 0;
    int rc;
    if ((rc = zkp::ctxop::grow_kzg(c, zkp::kzg::eval_layout(n_poly, log2_n).total, &ws)) || (rc = zkp::ctxop::kzg_domain(c, log2_n, &table, &table_log2, s)))
        return rc;
    return coop_rc(c, "fr_eval", zkp::fr_eval(ws, table, table_log2, (const uint64_t*)evals, (const uint64_t*)z, n_poly, log2_n, flags, (uint64_t*)out, s));
}
bool fr_eval_args_bad(const zkp_ctx* c, const void* evals, const void* z, size_t n_poly, unsigned log2_n, int flags, const void* out) {
    return !c || zkp::kzg::eval_args_bad(n_poly, log2_n, flags) || (n_poly && (!evals || !z || !out));
}
bool kzg_args_bad(const zkp_ctx* c, const zkp_kzg_vk* vk, const zkp_kzg_batch* b, const void* rand, int flags, const void* all_ok) {
    if (!c || !vk || !b || !all_ok || zkp::kzg::args_bad(b->n, flags)) return true;
    if (!b->n) return false;
    return !rand || !vk->g1 || !vk->g2 || !vk->tau_g2 || !b->c || !b->proof || !b->z || !b->y;
}
// validation mode: v(pointer, Fp count) over every coordinate array of the setup and the batch
template <class V>
int kzg_validate(const zkp_kzg_vk* vk, const zkp_kzg_batch* b, V&& v) {
    int rc;
    if ((rc = v(b->c, b->n * 2)) || (rc = v(b->proof, b->n * 2)) || (rc = v(vk->g1, 2)) || (rc = v(vk->g2, 4)) || (rc = v(vk->tau_g2, 4))) return rc;
    return ZKP_OK;
}
}  // namespace

extern "C" {

int zkp_fr_invert_batch_dev(zkp_ctx* c, const void* a, size_t n, void* out, void* stream) {
    if (!c || zkp::kzg::inv_args_bad(n) || (n && (!a || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    if (int rc = validate_fr_on_stream(c, a, n, S(stream))) return rc;
    return fr_invert_dev(c, a, n, out, S(stream));
}
int zkp_fr_invert_batch(zkp_ctx* c, const uint64_t* a, size_t n, uint64_t* out) {
    if (!c || zkp::kzg::inv_args_bad(n) || (n && (!a || !out))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    void* d = io.slot(0, n * 32);     // inverted in place on the device
    io.put(d, a, n * 32);
    io.get(out, d, n * 32);
    int rc;
    if ((rc = io.status()) || (rc = validate_fr_dev(c, d, n)) || (rc = fr_invert_dev(c, d, n, d, c->stream))) return rc;
    return io.finish();
}
int zkp_fr_eval_batch_dev(zkp_ctx* c, const void* evals, const void* z, size_t n_poly, unsigned log2_n, int flags, void* out, void* stream) {
    if (fr_eval_args_bad(c, evals, z, n_poly, log2_n, flags, out)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n_poly) return ZKP_OK;
    int rc;
    if ((rc = validate_fr_on_stream(c, evals, n_poly << log2_n, S(stream))) || (rc = validate_fr_on_stream(c, z, n_poly, S(stream)))) return rc;
    return fr_eval_dev(c, evals, z, n_poly, log2_n, flags, out, S(stream));
}
int zkp_fr_eval_batch(zkp_ctx* c, const uint64_t* evals, const uint64_t* z, size_t n_poly, unsigned log2_n, int flags, uint64_t* out) {
    if (fr_eval_args_bad(c, evals, z, n_poly, log2_n, flags, out)) return ZKP_ERR_ARG;
    if (!n_poly) return ZKP_OK;
    HostIO io(c);
    const void* de = io.in(0, evals, (n_poly << log2_n) * 32);
    const void* dz = io.in(1, z, n_poly * 32);
    void* dout = io.out(4, out, n_poly * 32);
    int rc;
    if ((rc = io.status()) || (rc = validate_fr_dev(c, de, n_poly << log2_n)) || (rc = validate_fr_dev(c, dz, n_poly)) ||
        (rc = fr_eval_dev(c, de, dz, n_poly, log2_n, flags, dout, c->stream)))
        return rc;
    return io.finish();
}
int zkp_kzg_verify_batch_dev(zkp_ctx* c, const zkp_kzg_vk* vk, const zkp_kzg_batch* b, const void* rand, int flags, void* all_ok, void* stream) {
    if (kzg_args_bad(c, vk, b, rand, flags, all_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (b->n)
        if (int rc = kzg_validate(vk, b, [&](const void* d, size_t n_fp) { return validate_on_stream(c, d, n_fp, S(stream)); })) return rc;
    return zkp::kzg_check_dev(c, vk, b, (const uint64_t*)rand, flags, (int*)all_ok, S(stream));
}
// the setup's and the batch's ten arrays one after the other in slot 0 (256-byte aligned), then the same driver as the _dev flavour
int zkp_kzg_verify_batch(zkp_ctx* c, const zkp_kzg_vk* vk, const zkp_kzg_batch* b, const uint64_t* rand, int flags, int* all_ok) {
    if (kzg_args_bad(c, vk, b, rand, flags, all_ok)) return ZKP_ERR_ARG;
    if (!b->n) { *all_ok = 1; return ZKP_OK; }
    const size_t n = b->n;
    zkp_kzg_vk dv = *vk;
    zkp_kzg_batch d = *b;
    const void* drand = rand;
    const void** field[10] = {&d.c, &d.inf_c, &d.proof, &d.inf_proof, &d.z, &d.y, &dv.g1, &dv.g2, &dv.tau_g2, &drand};
    const size_t bytes[10] = {n * 96, n, n * 96, n, n * 32, n * 32, 96, 192, 192, n * 16};
    size_t off[10], total = 0;
    for (int i = 0; i < 10; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    char* dev = (char*)io.slot(0, total);
    for (int i = 0; i < 10; i++) *field[i] = io.put(dev + off[i], *field[i], bytes[i]);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = kzg_validate(&dv, &d, [&](const void* p, size_t n_fp) { return validate_dev(c, (const uint64_t*)p, n_fp); })) ||
        (rc = zkp::kzg_check_dev(c, &dv, &d, (const uint64_t*)drand, flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- the batched Fr NTT and the KZG opening (zkp_poly.hip, include/zkp_poly.h)
namespace {
int fr_ntt_dev(zkp_ctx* c, const void* in, size_t n_poly, unsigned log2_n, int flags, void* out, hipStream_t s) {
    void* ws = nullptr;
    const uint32_t *table = nullptr, *coset = nullptr;
    unsigned table_log2 = 0;
    int rc;
    const size_t bytes = zkp::poly::ntt_workspace_bytes(n_poly, log2_n, flags);
    if ((bytes && (rc = zkp::ctxop::grow_kzg(c, bytes, &ws))) || (rc = zkp::ctxop::kzg_domain(c, log2_n, &table, &table_log2, s)) ||
        ((flags & ZKP_NTT_COSET) && (rc = zkp::ctxop::poly_coset(c, &coset, s))))
        return rc;
    return coop_rc(c, "fr_ntt", zkp::fr_ntt(ws, table, table_log2, coset, (const uint64_t*)in, n_poly, log2_n, flags, (uint64_t*)out, s));
}
bool fr_ntt_args_bad(const zkp_ctx* c, const void* in, size_t n_poly, unsigned log2_n, int flags, const void* out) {
    return !c || zkp::poly::ntt_args_bad(n_poly, log2_n, flags) || (n_poly && (!in || !out));
}
bool kzg_open_args_bad(const zkp_ctx* c, const void* lagrange, const void* evals, const void* z, size_t n, unsigned log2_n, int flags, const void* y,
                       const void* proof, const void* inf) {
    return !c || zkp::poly::open_args_bad(n, log2_n, flags) || (n && (!lagrange || !evals || !z || !y || !proof || !inf));
}
}  // namespace

extern "C" {

int zkp_fr_ntt_batch_dev(zkp_ctx* c, const void* in, size_t n_poly, unsigned log2_n, int flags, void* out, void* stream) {
    if (fr_ntt_args_bad(c, in, n_poly, log2_n, flags, out)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n_poly) return ZKP_OK;
    if (int rc = validate_fr_on_stream(c, in, n_poly << log2_n, S(stream))) return rc;
    return fr_ntt_dev(c, in, n_poly, log2_n, flags, out, S(stream));
}
int zkp_fr_ntt_batch(zkp_ctx* c, const uint64_t* in, size_t n_poly, unsigned log2_n, int flags, uint64_t* out) {
    if (fr_ntt_args_bad(c, in, n_poly, log2_n, flags, out)) return ZKP_ERR_ARG;
    if (!n_poly) return ZKP_OK;
    const size_t bytes = (n_poly << log2_n) * 32;
    HostIO io(c);
    void* d = io.slot(0, bytes);      // transformed in place on the device
    io.put(d, in, bytes);
    io.get(out, d, bytes);
    int rc;
    if ((rc = io.status()) || (rc = validate_fr_dev(c, d, n_poly << log2_n)) || (rc = fr_ntt_dev(c, d, n_poly, log2_n, flags, d, c->stream))) return rc;
    return io.finish();
}
int zkp_kzg_open_batch_dev(zkp_ctx* c, const void* lagrange, const void* evals, const void* z, size_t n, unsigned log2_n, int flags, void* out_y,
                           void* out_proof, void* out_inf, void* stream) {
    if (kzg_open_args_bad(c, lagrange, evals, z, n, log2_n, flags, out_y, out_proof, out_inf)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    int rc;
    if ((rc = validate_on_stream(c, lagrange, ((size_t)1 << log2_n) * 2, S(stream))) || (rc = validate_fr_on_stream(c, evals, n << log2_n, S(stream))) ||
        (rc = validate_fr_on_stream(c, z, n, S(stream))))
        return rc;
    return zkp::kzg_open_dev(c, lagrange, (const uint64_t*)evals, (const uint64_t*)z, n, log2_n, flags, (uint64_t*)out_y, (uint64_t*)out_proof,
                             (uint8_t*)out_inf, S(stream));
}
// the three outputs one after the other in slot 4 (256-byte aligned), then the same driver as the _dev flavour
int zkp_kzg_open_batch(zkp_ctx* c, const uint64_t* lagrange, const uint64_t* evals, const uint64_t* z, size_t n, unsigned log2_n, int flags, uint64_t* out_y,
                       uint64_t* out_proof, uint8_t* out_inf) {
    if (kzg_open_args_bad(c, lagrange, evals, z, n, log2_n, flags, out_y, out_proof, out_inf)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    const size_t N = (size_t)1 << log2_n, off_p = (n * 32 + 255) & ~(size_t)255, off_i = off_p + ((n * 96 + 255) & ~(size_t)255);
    HostIO io(c);
    const void* dl = io.in(0, lagrange, N * 96);
    const void* de = io.in(1, evals, (n << log2_n) * 32);
    const void* dz = io.in(2, z, n * 32);
    char* dout = (char*)io.slot(4, off_i + n);
    if (dout) {
        io.get(out_y, dout, n * 32);
        io.get(out_proof, dout + off_p, n * 96);
        io.get(out_inf, dout + off_i, n);
    }
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)dl, N * 2)) || (rc = validate_fr_dev(c, de, n << log2_n)) || (rc = validate_fr_dev(c, dz, n)) ||
        (rc = zkp::kzg_open_dev(c, dl, (const uint64_t*)de, (const uint64_t*)dz, n, log2_n, flags, (uint64_t*)dout, (uint64_t*)(dout + off_p),
                                (uint8_t*)(dout + off_i), c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- the Fr sparse product, the QAP quotient and the Groth16 prover (zkp_prove.hip,
// include/zkp_prove.h)
namespace {
bool csr_ptrs_bad(const zkp_fr_csr* m) { return (m->n_rows && !m->row_ptr) || (m->nnz && (!m->col || !m->val)); }
bool spmv_args_bad(const zkp_ctx* c, const zkp_fr_csr* m, const void* x, size_t n, size_t out_stride, const void* out) {
    if (!c || !m || zkp::prove::spmv_args_bad(m->n_rows, m->n_cols, m->nnz, n, out_stride) || csr_ptrs_bad(m)) return true;
    return n && ((out_stride && !out) || (m->n_cols && !x));
}
bool r1cs_args_bad(const zkp_ctx* c, const zkp_r1cs* r, const void* witness, size_t n) {
    if (!c || !r ||
        zkp::prove::r1cs_args_bad(r->log2_n, r->n_inputs, r->a.n_rows, r->a.n_cols, r->a.nnz, r->b.n_rows, r->b.n_cols, r->b.nnz, r->c.n_rows, r->c.n_cols,
                                  r->c.nnz, n) ||
        csr_ptrs_bad(&r->a) || csr_ptrs_bad(&r->b) || csr_ptrs_bad(&r->c))
        return true;
    return n && !witness;
}
bool prove_args_bad(const zkp_ctx* c, const zkp_r1cs* r, const zkp_groth16_pk* pk, const void* witness, const void* rs, size_t n, int flags, const void* a,
                    const void* ia, const void* b, const void* ib, const void* cc, const void* ic, const void* sat) {
    if (flags || !pk || r1cs_args_bad(c, r, witness, n)) return true;
    if (!n) return false;
    if (!rs || !a || !ia || !b || !ib || !cc || !ic || !sat) return true;
    if (!pk->alpha_g1 || !pk->beta_g1 || !pk->delta_g1 || !pk->beta_g2 || !pk->delta_g2 || !pk->a_query || !pk->b_g1_query || !pk->b_g2_query || !pk->h_query)
        return true;
    return r->a.n_cols - r->n_inputs - 1 && !pk->l_query;
}
// what the host flavour can check and the _dev flavour cannot: the row bounds and the columns of a matrix in host memory
bool csr_malformed(const zkp_fr_csr* m) {
    const uint32_t* rp = (const uint32_t*)m->row_ptr;
    const uint32_t* col = (const uint32_t*)m->col;
    if (m->n_rows) {
        if (rp[0] != 0 || rp[m->n_rows] != m->nnz) return true;
        for (size_t k = 0; k < m->n_rows; k++)
            if (rp[k] > rp[k + 1]) return true;
    } else if (m->nnz) {
        return true;
    }
    for (size_t e = 0; e < m->nnz; e++)
        if (col[e] >= m->n_cols) return true;
    return false;
}
// a matrix's three arrays into one workspace slot (256-byte aligned one after the other): *d is m with device pointers
size_t csr_bytes(const zkp_fr_csr* m) {
    return zkp::prove::up256((m->n_rows + 1) * 4) + zkp::prove::up256(m->nnz * 4) + zkp::prove::up256(m->nnz * 32);
}
char* csr_put(Staging& io, char* dev, const zkp_fr_csr* m, zkp_fr_csr* d) {
    *d = *m;
    d->row_ptr = m->n_rows ? io.put(dev, m->row_ptr, (m->n_rows + 1) * 4) : nullptr;
    dev += zkp::prove::up256((m->n_rows + 1) * 4);
    d->col = io.put(dev, m->col, m->nnz * 4);
    dev += zkp::prove::up256(m->nnz * 4);
    d->val = io.put(dev, m->val, m->nnz * 32);
    return dev + zkp::prove::up256(m->nnz * 32);
}
int spmv_dev(zkp_ctx* c, const zkp_fr_csr* m, const void* x, size_t n, size_t out_stride, void* out, hipStream_t s) {
    return coop_rc(c, "fr_spmv", zkp::fr_spmv(m, (const uint64_t*)x, n, out_stride, 0, (uint64_t*)out, c->d_flag + 2, s));
}
// validation mode: v(pointer, Fr count) over the values of the three matrices
template <class V>
int r1cs_validate(const zkp_r1cs* r, V&& v) {
    int rc;
    if ((rc = v(r->a.val, r->a.nnz)) || (rc = v(r->b.val, r->b.nnz)) || (rc = v(r->c.val, r->c.nnz))) return rc;
    return ZKP_OK;
}
// validation mode: v(pointer, Fp count) over every coordinate array of a proving key
template <class V>
int pk_validate(const zkp_r1cs* r, const zkp_groth16_pk* pk, V&& v) {
    const size_t m = r->a.n_cols, N = (size_t)1 << r->log2_n;
    int rc;
    if ((rc = v(pk->alpha_g1, 2)) || (rc = v(pk->beta_g1, 2)) || (rc = v(pk->delta_g1, 2)) || (rc = v(pk->beta_g2, 4)) || (rc = v(pk->delta_g2, 4)) ||
        (rc = v(pk->a_query, m * 2)) || (rc = v(pk->b_g1_query, m * 2)) || (rc = v(pk->b_g2_query, m * 4)) ||
        (rc = v(pk->l_query, (m - r->n_inputs - 1) * 2)) || (rc = v(pk->h_query, (N - 1) * 2)))
        return rc;
    return ZKP_OK;
}
}  // namespace

extern "C" {

int zkp_fr_spmv_batch_dev(zkp_ctx* c, const zkp_fr_csr* m, const void* x, size_t n, size_t out_stride, void* out, void* stream) {
    if (spmv_args_bad(c, m, x, n, out_stride, out)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n || !out_stride) return ZKP_OK;
    int rc;
    if ((rc = validate_fr_on_stream(c, m->val, m->nnz, S(stream))) || (rc = validate_fr_on_stream(c, x, n * m->n_cols, S(stream)))) return rc;
    return spmv_dev(c, m, x, n, out_stride, out, S(stream));
}
int zkp_fr_spmv_batch(zkp_ctx* c, const zkp_fr_csr* m, const uint64_t* x, size_t n, size_t out_stride, uint64_t* out) {
    if (spmv_args_bad(c, m, x, n, out_stride, out)) return ZKP_ERR_ARG;
    if (csr_malformed(m)) return ZKP_ERR_ARG;
    if (!n || !out_stride) return ZKP_OK;
    HostIO io(c);
    zkp_fr_csr d;
    char* dev = (char*)io.slot(0, csr_bytes(m));
    csr_put(io, dev, m, &d);
    const void* dx = io.in(1, x, n * m->n_cols * 32);
    void* dout = io.out(4, out, n * out_stride * 32);
    int rc;
    if ((rc = io.status()) || (rc = validate_fr_dev(c, d.val, d.nnz)) || (rc = validate_fr_dev(c, dx, n * m->n_cols)) ||
        (rc = spmv_dev(c, &d, dx, n, out_stride, dout, c->stream)))
        return rc;
    return io.finish();
}
int zkp_groth16_quotient_batch_dev(zkp_ctx* c, const zkp_r1cs* r, const void* witness, size_t n, void* out_h, void* out_sat, void* stream) {
    if (r1cs_args_bad(c, r, witness, n) || (n && (!out_h || !out_sat))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    int rc;
    if ((rc = r1cs_validate(r, [&](const void* d, size_t cnt) { return validate_fr_on_stream(c, d, cnt, S(stream)); })) ||
        (rc = validate_fr_on_stream(c, witness, n * r->a.n_cols, S(stream))))
        return rc;
    return zkp::groth16_quotient_dev(c, r, (const uint64_t*)witness, n, (uint64_t*)out_h, (uint8_t*)out_sat, S(stream));
}
// the three matrices one after the other in slot 0, the witness in slot 1, h and sat in slots 4 and 5, then the _dev flavour's driver
int zkp_groth16_quotient_batch(zkp_ctx* c, const zkp_r1cs* r, const uint64_t* witness, size_t n, uint64_t* out_h, uint8_t* out_sat) {
    if (r1cs_args_bad(c, r, witness, n) || (n && (!out_h || !out_sat))) return ZKP_ERR_ARG;
    if (csr_malformed(&r->a) || csr_malformed(&r->b) || csr_malformed(&r->c)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    const size_t m = r->a.n_cols, N = (size_t)1 << r->log2_n;
    HostIO io(c);
    zkp_r1cs d = *r;
    char* dev = (char*)io.slot(0, csr_bytes(&r->a) + csr_bytes(&r->b) + csr_bytes(&r->c));
    dev = csr_put(io, dev, &r->a, &d.a);
    dev = csr_put(io, dev, &r->b, &d.b);
    csr_put(io, dev, &r->c, &d.c);
    const void* dw = io.in(1, witness, n * m * 32);
    void* dh = io.out(4, out_h, n * N * 32);
    void* dsat = io.out(5, out_sat, n);
    int rc;
    if ((rc = io.status()) || (rc = r1cs_validate(&d, [&](const void* p, size_t cnt) { return validate_fr_dev(c, p, cnt); })) ||
        (rc = validate_fr_dev(c, dw, n * m)) || (rc = zkp::groth16_quotient_dev(c, &d, (const uint64_t*)dw, n, (uint64_t*)dh, (uint8_t*)dsat, c->stream)))
        return rc;
    return io.finish();
}
int zkp_groth16_prove_batch_dev(zkp_ctx* c, const zkp_r1cs* r, const zkp_groth16_pk* pk, const void* witness, const void* rs, size_t n, int flags,
                                void* out_a, void* out_inf_a, void* out_b, void* out_inf_b, void* out_c, void* out_inf_c, void* out_sat, void* stream) {
    if (prove_args_bad(c, r, pk, witness, rs, n, flags, out_a, out_inf_a, out_b, out_inf_b, out_c, out_inf_c, out_sat)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    int rc;
    if ((rc = r1cs_validate(r, [&](const void* d, size_t cnt) { return validate_fr_on_stream(c, d, cnt, S(stream)); })) ||
        (rc = validate_fr_on_stream(c, witness, n * r->a.n_cols, S(stream))) || (rc = validate_fr_on_stream(c, rs, n * 2, S(stream))) ||
        (rc = pk_validate(r, pk, [&](const void* d, size_t n_fp) { return validate_on_stream(c, d, n_fp, S(stream)); })))
        return rc;
    return zkp::groth16_prove_dev(c, r, pk, (const uint64_t*)witness, (const uint64_t*)rs, n, (uint64_t*)out_a, (uint8_t*)out_inf_a, (uint64_t*)out_b,
                                  (uint8_t*)out_inf_b, (uint64_t*)out_c, (uint8_t*)out_inf_c, (uint8_t*)out_sat, S(stream));
}
// the matrices in slot 0, the witness in slot 1, rs in slot 2, the key's fourteen arrays one after the other in slot 3, the seven
// outputs one after the other in slot 4 (everything 256-byte aligned), then the _dev flavour's driver
int zkp_groth16_prove_batch(zkp_ctx* c, const zkp_r1cs* r, const zkp_groth16_pk* pk, const uint64_t* witness, const uint64_t* rs, size_t n, int flags,
                            uint64_t* out_a, uint8_t* out_inf_a, uint64_t* out_b, uint8_t* out_inf_b, uint64_t* out_c, uint8_t* out_inf_c, uint8_t* out_sat) {
    if (prove_args_bad(c, r, pk, witness, rs, n, flags, out_a, out_inf_a, out_b, out_inf_b, out_c, out_inf_c, out_sat)) return ZKP_ERR_ARG;
    if (csr_malformed(&r->a) || csr_malformed(&r->b) || csr_malformed(&r->c)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    const size_t m = r->a.n_cols, N = (size_t)1 << r->log2_n, nl = m - r->n_inputs - 1;
    HostIO io(c);
    zkp_r1cs d = *r;
    char* dev = (char*)io.slot(0, csr_bytes(&r->a) + csr_bytes(&r->b) + csr_bytes(&r->c));
    dev = csr_put(io, dev, &r->a, &d.a);
    dev = csr_put(io, dev, &r->b, &d.b);
    csr_put(io, dev, &r->c, &d.c);
    const void* dw = io.in(1, witness, n * m * 32);
    const void* drs = io.in(2, rs, n * 64);
    zkp_groth16_pk dk = *pk;
    const void** field[14] = {&dk.alpha_g1, &dk.beta_g1, &dk.delta_g1, &dk.beta_g2, &dk.delta_g2, &dk.a_query, &dk.a_inf, &dk.b_g1_query, &dk.b_g1_inf,
                              &dk.b_g2_query, &dk.b_g2_inf, &dk.l_query, &dk.l_inf, &dk.h_query};
    const size_t bytes[14] = {96, 96, 96, 192, 192, m * 96, m, m * 96, m, m * 192, m, nl * 96, nl, (N - 1) * 96};
    size_t off[14], total = 0;
    for (int i = 0; i < 14; i++) {
        off[i] = total;
        total += zkp::prove::up256(bytes[i]);
    }
    char* dpk = (char*)io.slot(3, total);
    for (int i = 0; i < 14; i++) *field[i] = bytes[i] ? io.put(dpk + off[i], *field[i], bytes[i]) : nullptr;
    void* const host_out[7] = {out_a, out_inf_a, out_b, out_inf_b, out_c, out_inf_c, out_sat};
    const size_t out_bytes[7] = {n * 96, n, n * 192, n, n * 96, n, n};
    size_t out_off[7], out_total = 0;
    for (int i = 0; i < 7; i++) {
        out_off[i] = out_total;
        out_total += zkp::prove::up256(out_bytes[i]);
    }
    char* dout = (char*)io.slot(4, out_total);
    if (dout)
        for (int i = 0; i < 7; i++) io.get(host_out[i], dout + out_off[i], out_bytes[i]);
    int rc;
    if ((rc = io.status()) || (rc = r1cs_validate(&d, [&](const void* p, size_t cnt) { return validate_fr_dev(c, p, cnt); })) ||
        (rc = validate_fr_dev(c, dw, n * m)) || (rc = validate_fr_dev(c, drs, n * 2)) ||
        (rc = pk_validate(&d, &dk, [&](const void* p, size_t n_fp) { return validate_dev(c, (const uint64_t*)p, n_fp); })) ||
        (rc = zkp::groth16_prove_dev(c, &d, &dk, (const uint64_t*)dw, (const uint64_t*)drs, n, (uint64_t*)(dout + out_off[0]), (uint8_t*)(dout + out_off[1]),
                                     (uint64_t*)(dout + out_off[2]), (uint8_t*)(dout + out_off[3]), (uint64_t*)(dout + out_off[4]),
                                     (uint8_t*)(dout + out_off[5]), (uint8_t*)(dout + out_off[6]), c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- the G1 NTT and the FK20 proofs (zkp_fk20.hip, include/zkp_fk20.h)
namespace {
bool g1_ntt_args_bad(const zkp_ctx* c, const void* points, size_t n_vec, unsigned log2_n, int flags, const void* out, const void* out_inf) {
    return !c || zkp::fk20::g1ntt_args_bad(n_vec, log2_n, flags) || (n_vec && (!points || !out || !out_inf));
}
bool fk20_setup_args_bad(const zkp_ctx* c, const void* monomial, unsigned log2_n, const void* out, const void* out_inf) {
    return !c || zkp::fk20::setup_args_bad(log2_n) || !monomial || !out || !out_inf;
}
bool fk20_args_bad(const zkp_ctx* c, const void* setup, const void* coeffs, size_t n, unsigned log2_n, int flags, const void* proof, const void* inf) {
    return !c || zkp::fk20::fk20_args_bad(n, log2_n, flags) || (n && (!setup || !coeffs || !proof || !inf));
}
}  // namespace

extern "C" {

int zkp_g1_ntt_batch_dev(zkp_ctx* c, const void* points, const void* inf, size_t n_vec, unsigned log2_n, int flags, void* out, void* out_inf, void* stream) {
    if (g1_ntt_args_bad(c, points, n_vec, log2_n, flags, out, out_inf)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n_vec) return ZKP_OK;
    if (int rc = validate_on_stream(c, points, (n_vec << log2_n) * 2, S(stream))) return rc;
    return zkp::g1_ntt_dev(c, (const uint64_t*)points, (const uint8_t*)inf, n_vec, log2_n, flags, (uint64_t*)out, (uint8_t*)out_inf, S(stream));
}
// the points in slot 0, their flags in slot 1, the two outputs one after the other in slot 4, then the _dev flavour's driver
int zkp_g1_ntt_batch(zkp_ctx* c, const uint64_t* points, const uint8_t* inf, size_t n_vec, unsigned log2_n, int flags, uint64_t* out, uint8_t* out_inf) {
    if (g1_ntt_args_bad(c, points, n_vec, log2_n, flags, out, out_inf)) return ZKP_ERR_ARG;
    if (!n_vec) return ZKP_OK;
    const size_t n = n_vec << log2_n, off_i = zkp::fk20::up256(n * 96);
    HostIO io(c);
    const void* dp = io.in(0, points, n * 96);
    const void* di = io.in(1, inf, n);
    char* dout = (char*)io.slot(4, off_i + n);
    if (dout) {
        io.get(out, dout, n * 96);
        io.get(out_inf, dout + off_i, n);
    }
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)dp, n * 2)) ||
        (rc = zkp::g1_ntt_dev(c, (const uint64_t*)dp, (const uint8_t*)di, n_vec, log2_n, flags, (uint64_t*)dout, (uint8_t*)(dout + off_i), c->stream)))
        return rc;
    return io.finish();
}
int zkp_kzg_fk20_setup_dev(zkp_ctx* c, const void* monomial_g1, unsigned log2_n, void* out, void* out_inf, void* stream) {
    if (fk20_setup_args_bad(c, monomial_g1, log2_n, out, out_inf)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, monomial_g1, ((size_t)1 << log2_n) * 2, S(stream))) return rc;
    return zkp::fk20_setup_dev(c, (const uint64_t*)monomial_g1, log2_n, (uint64_t*)out, (uint8_t*)out_inf, S(stream));
}
int zkp_kzg_fk20_setup(zkp_ctx* c, const uint64_t* monomial_g1, unsigned log2_n, uint64_t* out, uint8_t* out_inf) {
    if (fk20_setup_args_bad(c, monomial_g1, log2_n, out, out_inf)) return ZKP_ERR_ARG;
    const size_t N = (size_t)1 << log2_n, off_i = zkp::fk20::up256(2 * N * 96);
    HostIO io(c);
    const void* dm = io.in(0, monomial_g1, N * 96);
    char* dout = (char*)io.slot(4, off_i + 2 * N);
    if (dout) {
        io.get(out, dout, 2 * N * 96);
        io.get(out_inf, dout + off_i, 2 * N);
    }
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)dm, N * 2)) ||
        (rc = zkp::fk20_setup_dev(c, (const uint64_t*)dm, log2_n, (uint64_t*)dout, (uint8_t*)(dout + off_i), c->stream)))
        return rc;
    return io.finish();
}
int zkp_kzg_fk20_batch_dev(zkp_ctx* c, const void* fk20_setup, const void* fk20_setup_inf, const void* coeffs, size_t n, unsigned log2_n, int flags,
                           void* out_proof, void* out_inf, void* stream) {
    if (fk20_args_bad(c, fk20_setup, coeffs, n, log2_n, flags, out_proof, out_inf)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    int rc;
    if ((rc = validate_on_stream(c, fk20_setup, ((size_t)2 << log2_n) * 2, S(stream))) || (rc = validate_fr_on_stream(c, coeffs, n << log2_n, S(stream)))) return rc;
    return zkp::fk20_dev(c, (const uint64_t*)fk20_setup, (const uint8_t*)fk20_setup_inf, (const uint64_t*)coeffs, n, log2_n, flags, (uint64_t*)out_proof,
                         (uint8_t*)out_inf, S(stream));
}
// the setup in slot 0, its flags in slot 1, the coefficients in slot 2, the two outputs one after the other in slot 4
int zkp_kzg_fk20_batch(zkp_ctx* c, const uint64_t* fk20_setup, const uint8_t* fk20_setup_inf, const uint64_t* coeffs, size_t n, unsigned log2_n, int flags,
                       uint64_t* out_proof, uint8_t* out_inf) {
    if (fk20_args_bad(c, fk20_setup, coeffs, n, log2_n, flags, out_proof, out_inf)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    const size_t N = (size_t)1 << log2_n, off_i = zkp::fk20::up256(n * N * 96);
    HostIO io(c);
    const void* ds = io.in(0, fk20_setup, 2 * N * 96);
    const void* dsi = io.in(1, fk20_setup_inf, 2 * N);
    const void* dc = io.in(2, coeffs, n * N * 32);
    char* dout = (char*)io.slot(4, off_i + n * N);
    if (dout) {
        io.get(out_proof, dout, n * N * 96);
        io.get(out_inf, dout + off_i, n * N);
    }
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)ds, 2 * N * 2)) || (rc = validate_fr_dev(c, dc, n * N)) ||
        (rc = zkp::fk20_dev(c, (const uint64_t*)ds, (const uint8_t*)dsi, (const uint64_t*)dc, n, log2_n, flags, (uint64_t*)dout, (uint8_t*)(dout + off_i),
                            c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- the KZG cell proofs (zkp_cells.hip, include/zkp_cells.h)
namespace {
bool cells_setup_args_bad(const zkp_ctx* c, const void* monomial, unsigned log2_n, unsigned log2_l, const void* out, const void* out_inf) {
    return !c || zkp::cells::setup_args_bad(log2_n, log2_l) || !monomial || !out || !out_inf;
}
zkp::CellBatch cell_batch_of(const void* monomial, const void* g2, const void* tau_l_g2, const void* cm, const void* inf_c, const void* index, const void* values,
                             const void* proofs, const void* inf_proof, size_t n, unsigned log2_d, unsigned log2_l, const void* rand) {
    zkp::CellBatch b;
    b.monomial = (const uint64_t*)monomial;
    b.g2 = (const uint64_t*)g2;
    b.tau_l_g2 = (const uint64_t*)tau_l_g2;
    b.c = (const uint64_t*)cm;
    b.values = (const uint64_t*)values;
    b.proof = (const uint64_t*)proofs;
    b.rand = (const uint64_t*)rand;
    b.inf_c = (const uint8_t*)inf_c;
    b.inf_proof = (const uint8_t*)inf_proof;
    b.index = (const uint32_t*)index;
    b.n = n;
    b.log2_d = log2_d;
    b.log2_l = log2_l;
    return b;
}
bool cell_verify_args_bad(const zkp_ctx* c, const zkp::CellBatch& b, int flags, const void* out_ok) {
    if (!c || !out_ok || zkp::cells::verify_args_bad(b.n, b.log2_d, b.log2_l, flags)) return true;
    if (!b.n) return false;
    return !b.monomial || !b.g2 || !b.tau_l_g2 || !b.c || !b.index || !b.values || !b.proof || !b.rand;
}
// validation mode: v(pointer, Fp count) over every coordinate array of the setup and the batch
template <class V>
int cell_validate(const zkp::CellBatch& b, V&& v) {
    int rc;
    if ((rc = v(b.c, b.n * 2)) || (rc = v(b.proof, b.n * 2)) || (rc = v(b.monomial, ((size_t)2 << b.log2_l))) || (rc = v(b.g2, 4)) || (rc = v(b.tau_l_g2, 4))) return rc;
    return ZKP_OK;
}
bool cells_args_bad(const zkp_ctx* c, const void* setup, const void* coeffs, size_t n, unsigned log2_n, unsigned log2_l, unsigned log2_ext, int flags,
                    const void* proof, const void* inf) {
    return !c || zkp::cells::cells_args_bad(n, log2_n, log2_l, log2_ext, flags) || (n && (!setup || !coeffs || !proof || !inf));
}
}  // namespace

extern "C" {

int zkp_kzg_cells_setup_dev(zkp_ctx* c, const void* monomial_g1, unsigned log2_n, unsigned log2_l, void* out, void* out_inf, void* stream) {
    if (cells_setup_args_bad(c, monomial_g1, log2_n, log2_l, out, out_inf)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, monomial_g1, ((size_t)1 << log2_n) * 2, S(stream))) return rc;
    return zkp::cells_setup_dev(c, (const uint64_t*)monomial_g1, log2_n, log2_l, (uint64_t*)out, (uint8_t*)out_inf, S(stream));
}
int zkp_kzg_cells_setup(zkp_ctx* c, const uint64_t* monomial_g1, unsigned log2_n, unsigned log2_l, uint64_t* out, uint8_t* out_inf) {
    if (cells_setup_args_bad(c, monomial_g1, log2_n, log2_l, out, out_inf)) return ZKP_ERR_ARG;
    const size_t N = (size_t)1 << log2_n, off_i = zkp::fk20::up256(2 * N * 96);
    HostIO io(c);
    const void* dm = io.in(0, monomial_g1, N * 96);
    char* dout = (char*)io.slot(4, off_i + 2 * N);
    if (dout) {
        io.get(out, dout, 2 * N * 96);
        io.get(out_inf, dout + off_i, 2 * N);
    }
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)dm, N * 2)) ||
        (rc = zkp::cells_setup_dev(c, (const uint64_t*)dm, log2_n, log2_l, (uint64_t*)dout, (uint8_t*)(dout + off_i), c->stream)))
        return rc;
    return io.finish();
}
int zkp_kzg_cells_batch_dev(zkp_ctx* c, const void* cells_setup, const void* cells_setup_inf, const void* coeffs, size_t n, unsigned log2_n, unsigned log2_l,
                            unsigned log2_ext, int flags, void* out_proof, void* out_inf, void* stream) {
    if (cells_args_bad(c, cells_setup, coeffs, n, log2_n, log2_l, log2_ext, flags, out_proof, out_inf)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    int rc;
    if ((rc = validate_on_stream(c, cells_setup, ((size_t)2 << log2_n) * 2, S(stream))) || (rc = validate_fr_on_stream(c, coeffs, n << log2_n, S(stream)))) return rc;
    return zkp::cells_dev(c, (const uint64_t*)cells_setup, (const uint8_t*)cells_setup_inf, (const uint64_t*)coeffs, n, log2_n, log2_l, log2_ext, flags,
                          (uint64_t*)out_proof, (uint8_t*)out_inf, S(stream));
}
// the setup in slot 0, its flags in slot 1, the coefficients in slot 2, the two outputs one after the other in slot 4
int zkp_kzg_cells_batch(zkp_ctx* c, const uint64_t* cells_setup, const uint8_t* cells_setup_inf, const uint64_t* coeffs, size_t n, unsigned log2_n,
                        unsigned log2_l, unsigned log2_ext, int flags, uint64_t* out_proof, uint8_t* out_inf) {
    if (cells_args_bad(c, cells_setup, coeffs, n, log2_n, log2_l, log2_ext, flags, out_proof, out_inf)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    const size_t N = (size_t)1 << log2_n, nm = n << (log2_n - log2_l + log2_ext), off_i = zkp::fk20::up256(nm * 96);
    HostIO io(c);
    const void* ds = io.in(0, cells_setup, 2 * N * 96);
    const void* dsi = io.in(1, cells_setup_inf, 2 * N);
    const void* dc = io.in(2, coeffs, n * N * 32);
    char* dout = (char*)io.slot(4, off_i + nm);
    if (dout) {
        io.get(out_proof, dout, nm * 96);
        io.get(out_inf, dout + off_i, nm);
    }
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)ds, 2 * N * 2)) || (rc = validate_fr_dev(c, dc, n * N)) ||
        (rc = zkp::cells_dev(c, (const uint64_t*)ds, (const uint8_t*)dsi, (const uint64_t*)dc, n, log2_n, log2_l, log2_ext, flags, (uint64_t*)dout,
                             (uint8_t*)(dout + off_i), c->stream)))
        return rc;
    return io.finish();
}

int zkp_kzg_cell_verify_batch_dev(zkp_ctx* c, const void* monomial_g1_l, const void* g2, const void* tau_l_g2, const void* commitments, const void* inf_c,
                                  const void* cell_index, const void* values, const void* proofs, const void* inf_proof, size_t n, unsigned log2_d,
                                  unsigned log2_l, int flags, const void* rand, void* out_ok, void* stream) {
    const zkp::CellBatch b = cell_batch_of(monomial_g1_l, g2, tau_l_g2, commitments, inf_c, cell_index, values, proofs, inf_proof, n, log2_d, log2_l, rand);
    if (cell_verify_args_bad(c, b, flags, out_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (n)
        if (int rc = cell_validate(b, [&](const void* d, size_t n_fp) { return validate_on_stream(c, d, n_fp, S(stream)); })) return rc;
    return zkp::cell_check_dev(c, b, flags, (int*)out_ok, S(stream));
}
// the ten arrays one after the other in slot 0 (256-byte aligned), then the same driver as the _dev flavour
int zkp_kzg_cell_verify_batch(zkp_ctx* c, const uint64_t* monomial_g1_l, const uint64_t* g2, const uint64_t* tau_l_g2, const uint64_t* commitments,
                              const uint8_t* inf_c, const uint32_t* cell_index, const uint64_t* values, const uint64_t* proofs, const uint8_t* inf_proof, size_t n,
                              unsigned log2_d, unsigned log2_l, int flags, const uint64_t* rand, int* out_ok) {
    zkp::CellBatch d = cell_batch_of(monomial_g1_l, g2, tau_l_g2, commitments, inf_c, cell_index, values, proofs, inf_proof, n, log2_d, log2_l, rand);
    if (cell_verify_args_bad(c, d, flags, out_ok)) return ZKP_ERR_ARG;
    if (!n) { *out_ok = 1; return ZKP_OK; }
    const size_t l = (size_t)1 << log2_l;
    const void* src[10] = {d.c, d.inf_c, d.proof, d.inf_proof, d.index, d.values, d.monomial, d.g2, d.tau_l_g2, d.rand};
    const size_t bytes[10] = {n * 96, n, n * 96, n, n * 4, n * l * 32, l * 96, 192, 192, n * 16};
    const void* dev_of[10];
    size_t off[10], total = 0;
    for (int i = 0; i < 10; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    char* dev = (char*)io.slot(0, total);
    for (int i = 0; i < 10; i++) dev_of[i] = io.put(dev + off[i], src[i], bytes[i]);
    d = cell_batch_of(dev_of[6], dev_of[7], dev_of[8], dev_of[0], dev_of[1], dev_of[4], dev_of[5], dev_of[2], dev_of[3], n, log2_d, log2_l, dev_of[9]);
    io.get(out_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = cell_validate(d, [&](const void* p, size_t n_fp) { return validate_dev(c, (const uint64_t*)p, n_fp); })) ||
        (rc = zkp::cell_check_dev(c, d, flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- the cell recovery (zkp_recover.hip, include/zkp_recover.h)
namespace {
bool recover_args_bad(const zkp_ctx* c, const void* values, const void* present, size_t n, unsigned log2_n, unsigned log2_l, int flags, const void* coeffs,
                      const void* ok) {
    return !c || zkp::rec::args_bad(n, log2_n, log2_l, flags) || (n && (!values || !present || !coeffs || !ok));
}
}  // namespace

extern "C" {

int zkp_das_recover_batch_dev(zkp_ctx* c, const void* values, const void* present, size_t n, unsigned log2_n, unsigned log2_l, int flags, void* out_coeffs,
                              void* out_ok, void* stream) {
    if (recover_args_bad(c, values, present, n, log2_n, log2_l, flags, out_coeffs, out_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (!n) return ZKP_OK;
    if (c->validate)
        HIPCHK(c, zkp::rec_check_present((const uint64_t*)values, (const uint8_t*)present, n << (log2_n + 1 - log2_l), log2_l, c->d_flag + 2, S(stream)));
    return zkp::recover_dev(c, (const uint64_t*)values, (const uint8_t*)present, n, log2_n, log2_l, flags, (uint64_t*)out_coeffs, (int32_t*)out_ok, S(stream));
}
// the values in slot 0, the mask in slot 1, the two outputs one after the other in slot 4
int zkp_das_recover_batch(zkp_ctx* c, const uint64_t* values, const uint8_t* present, size_t n, unsigned log2_n, unsigned log2_l, int flags,
                          uint64_t* out_coeffs, int32_t* out_ok) {
    if (recover_args_bad(c, values, present, n, log2_n, log2_l, flags, out_coeffs, out_ok)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    const size_t rows = n << (log2_n + 1 - log2_l), off_ok = zkp::kzg::align256((n << log2_n) * 32);
    HostIO io(c);
    const void* dv = io.in(0, values, (rows << log2_l) * 32);
    const void* dp = io.in(1, present, rows);
    char* dout = (char*)io.slot(4, off_ok + n * sizeof(int32_t));
    if (dout) {
        io.get(out_coeffs, dout, (n << log2_n) * 32);
        io.get(out_ok, dout + off_ok, n * sizeof(int32_t));
    }
    int rc;
    if ((rc = io.status())) return rc;
    if (c->validate) {
        HIPCHK(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), c->stream));
        HIPCHK(c, zkp::rec_check_present((const uint64_t*)dv, (const uint8_t*)dp, rows, log2_l, c->d_flag, c->stream));
        int bad = 0;
        HIPCHK(c, hipMemcpyAsync(&bad, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (bad) { c->err = "input limbs >= r"; return ZKP_ERR_NONCANONICAL; }
    }
    if ((rc = zkp::recover_dev(c, (const uint64_t*)dv, (const uint8_t*)dp, n, log2_n, log2_l, flags, (uint64_t*)dout, (int32_t*)(dout + off_ok), c->stream))) return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- hash-to-G2 and the BLS batch verifier (zkp_bls.hip, include/zkp_bls.h)
namespace {
bool h2c_msgs_bad(const zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len) {
    (void)msgs;   // may be null: every message may be empty
    return !c || n > zkp::bls::MAX_N || zkp::bls::dst_bad(dst_len) || !dst || (n && !offsets);
}
// host offsets: non-decreasing, and a buffer behind them when any message has a byte
bool offsets_malformed(const uint8_t* msgs, const uint64_t* offsets, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return true;
    return n && offsets[n] > offsets[0] && !msgs;
}
// the messages of a host call in workspace slots: the bytes [offsets[0], offsets[n]) in slot `sb`, the offsets in slot `so`, the DST in `sd`;
// *dmsgs is biased so that the caller's offsets index it
void stage_msgs(Staging& io, int sb, int so, int sd, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len,
                const uint8_t** dmsgs, const void** doff, const void** ddst) {
    const uint64_t lo = n ? offsets[0] : 0, bytes = n ? offsets[n] - offsets[0] : 0;
    const uint8_t* db = bytes ? (const uint8_t*)io.in(sb, msgs + lo, bytes) : nullptr;
    *dmsgs = db ? db - lo : nullptr;
    *doff = io.in(so, offsets, (n + 1) * 8);
    *ddst = io.in(sd, dst, dst_len);
}
}  // namespace

extern "C" {

int zkp_fp_from_wide_be_batch_dev(zkp_ctx* c, const void* bytes, size_t n, void* out, void* stream) {
    if (!c || n > zkp::bls::MAX_N || (n && (!bytes || !out))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return zkp::h2c_wide_dev(c, bytes, n, out, S(stream));
}
int zkp_fp_from_wide_be_batch(zkp_ctx* c, const uint8_t* bytes, size_t n, uint64_t* out) {
    if (!c || n > zkp::bls::MAX_N || (n && (!bytes || !out))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const void* din = io.in(0, bytes, n * 64);
    void* dout = io.out(4, out, n * 48);
    int rc;
    if ((rc = io.status()) || (rc = zkp::h2c_wide_dev(c, din, n, dout, c->stream))) return rc;
    return io.finish();
}

int zkp_hash_to_field_g2_batch_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out_u, void* stream) {
    if (h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || (n && !out_u)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return zkp::h2c_field_dev(c, msgs, offsets, n, dst, dst_len, out_u, S(stream));
}
int zkp_hash_to_field_g2_batch(zkp_ctx* c, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len, uint64_t* out_u) {
    if (h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || (n && !out_u) || offsets_malformed(msgs, offsets, n)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n, dst, dst_len, &dm, &dof, &dd);
    void* dout = io.out(4, out_u, n * 192);
    int rc;
    if ((rc = io.status()) || (rc = zkp::h2c_field_dev(c, dm, dof, n, dd, dst_len, dout, c->stream))) return rc;
    return io.finish();
}

int zkp_g2_map_from_fields_batch_dev(zkp_ctx* c, const void* u, size_t n, void* out, void* out_inf, void* stream) {
    if (!c || n > zkp::bls::MAX_N || (n && (!u || !out || !out_inf))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, u, n * 4, S(stream))) return rc;
    return zkp::h2c_map_dev(c, u, n, out, out_inf, S(stream));
}
int zkp_g2_map_from_fields_batch(zkp_ctx* c, const uint64_t* u, size_t n, uint64_t* out, uint8_t* out_inf) {
    if (!c || n > zkp::bls::MAX_N || (n && (!u || !out || !out_inf))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const void* du = io.in(0, u, n * 192);
    void* dout = io.out(4, out, n * 192);
    void* dinf = io.out(6, out_inf, n);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)du, n * 4)) || (rc = zkp::h2c_map_dev(c, du, n, dout, dinf, c->stream))) return rc;
    return io.finish();
}

int zkp_g2_clear_cofactor_batch_dev(zkp_ctx* c, const void* pts, const void* inf, size_t n, void* out, void* out_inf, void* stream) {
    if (!c || n > zkp::bls::MAX_N || (n && (!pts || !out || !out_inf))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, pts, n * 4, S(stream))) return rc;
    return zkp::h2c_clear_dev(c, pts, inf, n, out, out_inf, S(stream));
}
int zkp_g2_clear_cofactor_batch(zkp_ctx* c, const uint64_t* pts, const uint8_t* inf, size_t n, uint64_t* out, uint8_t* out_inf) {
    if (!c || n > zkp::bls::MAX_N || (n && (!pts || !out || !out_inf))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const void* dp = io.in(0, pts, n * 192);
    const void* di = io.in(2, inf, n);
    void* dout = io.out(4, out, n * 192);
    void* dinf = io.out(6, out_inf, n);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)dp, n * 4)) || (rc = zkp::h2c_clear_dev(c, dp, di, n, dout, dinf, c->stream))) return rc;
    return io.finish();
}

int zkp_hash_to_g2_batch_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out, void* out_inf,
                             void* stream) {
    if (h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || (n && (!out || !out_inf))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return zkp::h2c_hash_dev(c, msgs, offsets, n, dst, dst_len, out, out_inf, S(stream));
}
int zkp_hash_to_g2_batch(zkp_ctx* c, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len, uint64_t* out,
                         uint8_t* out_inf) {
    if (h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || (n && (!out || !out_inf)) || offsets_malformed(msgs, offsets, n)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n, dst, dst_len, &dm, &dof, &dd);
    void* dout = io.out(4, out, n * 192);
    void* dinf = io.out(6, out_inf, n);
    int rc;
    if ((rc = io.status()) || (rc = zkp::h2c_hash_dev(c, dm, dof, n, dd, dst_len, dout, dinf, c->stream))) return rc;
    return io.finish();
}

static bool bls_args_bad(const zkp_ctx* c, const void* pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig, size_t n,
                         const void* rand, int flags, const void* all_ok) {
    return h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || !all_ok || (flags & ~ZKP_BLS_POINTS_CHECKED) || n > zkp::bls::MAX_VERIFY_N ||
           zkp::rlc::args_bad(n, 1, 1, 0) || (n && (!pk || !sig || !rand));
}
int zkp_bls_verify_batch_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len,
                             const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, void* all_ok, void* stream) {
    if (bls_args_bad(c, pk, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int rc;
    if ((rc = validate_on_stream(c, pk, n * 2, S(stream))) || (rc = validate_on_stream(c, sig, n * 4, S(stream)))) return rc;
    return zkp::bls_verify_dev(c, pk, inf_pk, msgs, offsets, dst, dst_len, sig, inf_sig, n, rand, flags, (int*)all_ok, S(stream));
}
// the seven arrays of points one after the other in slot 3 (256-byte aligned), the messages in slots 0..2, then the same driver
int zkp_bls_verify_batch(zkp_ctx* c, const uint64_t* pk, const uint8_t* inf_pk, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst,
                         size_t dst_len, const uint64_t* sig, const uint8_t* inf_sig, size_t n, const uint64_t* rand, int flags, int* all_ok) {
    if (bls_args_bad(c, pk, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok) || offsets_malformed(msgs, offsets, n)) return ZKP_ERR_ARG;
    if (!n) { *all_ok = 1; return ZKP_OK; }
    const void* field[5] = {pk, inf_pk, sig, inf_sig, rand};
    const size_t bytes[5] = {n * 96, n, n * 192, n, n * 16};
    size_t off[5], total = 0;
    for (int i = 0; i < 5; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n, dst, dst_len, &dm, &dof, &dd);
    char* dev = (char*)io.slot(3, total);
    const void* d[5];
    for (int i = 0; i < 5; i++) d[i] = io.put(dev + off[i], field[i], bytes[i]);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)d[0], n * 2)) || (rc = validate_dev(c, (const uint64_t*)d[2], n * 4)) ||
        (rc = zkp::bls_verify_dev(c, d[0], d[1], dm, dof, dd, dst_len, d[2], d[3], n, d[4], flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- G1 segment sums and FastAggregateVerify (zkp_bls_agg.hip, include/zkp_bls_agg.h)
namespace {
bool agg_sum_args_bad(const zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, const void* out,
                      const void* out_inf, const void* status) {
    return !c || zkp::agg::args_bad(n_table, n_idx, n_seg) || (n_table && !table) || (n_idx && !idx) || ((n_seg || n_idx) && !seg_off) ||
           (n_seg && (!out || !out_inf || !status));
}
bool agg_verify_args_bad(const zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* msgs,
                         const void* offsets, const void* dst, size_t dst_len, const void* sig, size_t n, const void* rand, int flags, const void* all_ok) {
    return h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || !all_ok || (flags & ~ZKP_BLS_POINTS_CHECKED) || n > zkp::bls::MAX_VERIFY_N ||
           zkp::rlc::args_bad(n, 1, 1, 0) || (n && (!sig || !rand)) || zkp::agg::args_bad(n_table, n_idx, n) || (n_table && !table) || (n_idx && !idx) ||
           ((n || n_idx) && !seg_off);
}
}  // namespace

extern "C" {

int zkp_g1_segment_sum_batch_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, void* out,
                                 void* out_inf, void* status, void* stream) {
    if (agg_sum_args_bad(c, table, n_table, idx, n_idx, seg_off, n_seg, out, out_inf, status)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, table, n_table * 2, S(stream))) return rc;
    return zkp::agg_segment_sum_dev(c, table, n_table, idx, n_idx, seg_off, n_seg, out, out_inf, status, S(stream));
}
int zkp_g1_segment_sum_batch(zkp_ctx* c, const uint64_t* table, size_t n_table, const uint32_t* idx, size_t n_idx, const uint64_t* seg_off, size_t n_seg,
                             uint64_t* out, uint8_t* out_inf, uint8_t* status) {
    if (agg_sum_args_bad(c, table, n_table, idx, n_idx, seg_off, n_seg, out, out_inf, status)) return ZKP_ERR_ARG;
    if (!n_seg && !n_idx) return ZKP_OK;
    if (zkp::agg::offsets_malformed(seg_off, n_seg, n_idx) || zkp::agg::rows_out_of_range(idx, n_idx, n_table)) return ZKP_ERR_ARG;
    HostIO io(c);
    const void* dt = io.in(0, table, n_table * 96);
    const void* di = io.in(1, idx, n_idx * 4);
    const void* ds = io.in(2, seg_off, (n_seg + 1) * 8);
    void* dout = io.out(4, out, n_seg * 96);
    void* dinf = io.out(5, out_inf, n_seg);
    void* dst = io.out(6, status, n_seg);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)dt, n_table * 2)) ||
        (rc = zkp::agg_segment_sum_dev(c, dt, n_table, di, n_idx, ds, n_seg, dout, dinf, dst, c->stream)))
        return rc;
    return io.finish();
}

int zkp_bls_fast_aggregate_verify_batch_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* msgs,
                                            const void* offsets, const void* dst, size_t dst_len, const void* sig, const void* inf_sig, size_t n,
                                            const void* rand, int flags, void* all_ok, void* stream) {
    if (agg_verify_args_bad(c, table, n_table, idx, n_idx, seg_off, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int rc;
    if ((rc = validate_on_stream(c, table, n_table * 2, S(stream))) || (rc = validate_on_stream(c, sig, n * 4, S(stream)))) return rc;
    return zkp::agg_verify_dev(c, table, n_table, idx, n_idx, seg_off, msgs, offsets, dst, dst_len, sig, inf_sig, n, rand, flags, (int*)all_ok, S(stream));
}
// the six arrays one after the other in slot 3 (256-byte aligned), the messages in slots 0..2, then the same driver
int zkp_bls_fast_aggregate_verify_batch(zkp_ctx* c, const uint64_t* table, size_t n_table, const uint32_t* idx, size_t n_idx, const uint64_t* seg_off,
                                        const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len, const uint64_t* sig,
                                        const uint8_t* inf_sig, size_t n, const uint64_t* rand, int flags, int* all_ok) {
    if (agg_verify_args_bad(c, table, n_table, idx, n_idx, seg_off, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok) ||
        offsets_malformed(msgs, offsets, n))
        return ZKP_ERR_ARG;
    if ((n || n_idx) && (zkp::agg::offsets_malformed(seg_off, n, n_idx) || zkp::agg::rows_out_of_range(idx, n_idx, n_table))) return ZKP_ERR_ARG;
    if (!n) { *all_ok = 1; return ZKP_OK; }
    const void* field[6] = {table, idx, seg_off, sig, inf_sig, rand};
    const size_t bytes[6] = {n_table * 96, n_idx * 4, (n + 1) * 8, n * 192, n, n * 16};
    size_t off[6], total = 0;
    for (int i = 0; i < 6; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n, dst, dst_len, &dm, &dof, &dd);
    char* dev = (char*)io.slot(3, total);
    const void* d[6];
    for (int i = 0; i < 6; i++) d[i] = io.put(dev + off[i], field[i], bytes[i]);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)d[0], n_table * 2)) || (rc = validate_dev(c, (const uint64_t*)d[3], n * 4)) ||
        (rc = zkp::agg_verify_dev(c, d[0], n_table, d[1], n_idx, d[2], dm, dof, dd, dst_len, d[3], d[4], n, d[5], flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- scaled G1 segment sums and the verifiers grouped by message (zkp_bls_grouped.hip,
// include/zkp_bls_grouped.h)
namespace {
bool grp_sum_args_bad(const zkp_ctx* c, const void* pts, const void* rand, size_t n, const void* seg_off, size_t n_seg, const void* out, const void* out_inf,
                      const void* status) {
    return !c || zkp::grp::args_bad(n, n_seg) || (n && (!pts || !rand)) || ((n_seg || n) && !seg_off) || (n_seg && (!out || !out_inf || !status));
}
bool grp_verify_args_bad(const zkp_ctx* c, const void* pk, const void* grp_off, const void* msgs, const void* offsets, size_t m, const void* dst, size_t dst_len,
                         const void* sig, size_t n, const void* rand, int flags, const void* all_ok) {
    return h2c_msgs_bad(c, msgs, offsets, m, dst, dst_len) || !all_ok || (flags & ~ZKP_BLS_POINTS_CHECKED) || zkp::grp::args_bad(n, m) ||
           n > zkp::bls::MAX_VERIFY_N || (n && zkp::rlc::args_bad(n, 1, 1, 0)) || (n && (!pk || !sig || !rand || !grp_off));
}
bool grp_fav_args_bad(const zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* grp_off,
                      const void* msgs, const void* offsets, size_t m, const void* dst, size_t dst_len, const void* sig, size_t n, const void* rand, int flags,
                      const void* all_ok) {
    return grp_verify_args_bad(c, sig, grp_off, msgs, offsets, m, dst, dst_len, sig, n, rand, flags, all_ok) || zkp::agg::args_bad(n_table, n_idx, n) ||
           (n_table && !table) || (n_idx && !idx) || ((n || n_idx) && !seg_off);
}
}  // namespace

extern "C" {

int zkp_g1_scaled_segment_sum_batch_dev(zkp_ctx* c, const void* pts, const void* inf, const void* rand, size_t n, const void* seg_off, size_t n_seg, void* out,
                                        void* out_inf, void* status, void* stream) {
    if (grp_sum_args_bad(c, pts, rand, n, seg_off, n_seg, out, out_inf, status)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, pts, n * 2, S(stream))) return rc;
    return zkp::grp_scaled_segment_sum_dev(c, pts, inf, rand, n, seg_off, n_seg, out, out_inf, status, S(stream));
}
int zkp_g1_scaled_segment_sum_batch(zkp_ctx* c, const uint64_t* pts, const uint8_t* inf, const uint64_t* rand, size_t n, const uint64_t* seg_off, size_t n_seg,
                                    uint64_t* out, uint8_t* out_inf, uint8_t* status) {
    if (grp_sum_args_bad(c, pts, rand, n, seg_off, n_seg, out, out_inf, status)) return ZKP_ERR_ARG;
    if (!n_seg && !n) return ZKP_OK;
    if (zkp::grp::offsets_malformed(seg_off, n_seg, n)) return ZKP_ERR_ARG;
    HostIO io(c);
    const void* dp = io.in(0, pts, n * 96);
    const void* dr = io.in(1, rand, n * 16);
    const void* ds = io.in(2, seg_off, (n_seg + 1) * 8);
    const void* di = io.in(3, inf, n);
    void* dout = io.out(4, out, n_seg * 96);
    void* dinf = io.out(5, out_inf, n_seg);
    void* dst = io.out(6, status, n_seg);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)dp, n * 2)) ||
        (rc = zkp::grp_scaled_segment_sum_dev(c, dp, di, dr, n, ds, n_seg, dout, dinf, dst, c->stream)))
        return rc;
    return io.finish();
}

int zkp_bls_verify_grouped_batch_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* grp_off, const void* msgs, const void* offsets, size_t m,
                                     const void* dst, size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, void* all_ok,
                                     void* stream) {
    if (grp_verify_args_bad(c, pk, grp_off, msgs, offsets, m, dst, dst_len, sig, n, rand, flags, all_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int rc;
    if ((rc = validate_on_stream(c, pk, n * 2, S(stream))) || (rc = validate_on_stream(c, sig, n * 4, S(stream)))) return rc;
    return zkp::grp_verify_dev(c, pk, inf_pk, grp_off, msgs, offsets, m, dst, dst_len, sig, inf_sig, n, rand, flags, (int*)all_ok, S(stream));
}
// the six arrays one after the other in slot 3 (256-byte aligned), the messages in slots 0..2, then the same driver
int zkp_bls_verify_grouped_batch(zkp_ctx* c, const uint64_t* pk, const uint8_t* inf_pk, const uint64_t* grp_off, const uint8_t* msgs, const uint64_t* offsets,
                                 size_t m, const uint8_t* dst, size_t dst_len, const uint64_t* sig, const uint8_t* inf_sig, size_t n, const uint64_t* rand,
                                 int flags, int* all_ok) {
    if (grp_verify_args_bad(c, pk, grp_off, msgs, offsets, m, dst, dst_len, sig, n, rand, flags, all_ok) || offsets_malformed(msgs, offsets, m)) return ZKP_ERR_ARG;
    if (grp_off && zkp::grp::offsets_malformed(grp_off, m, n)) return ZKP_ERR_ARG;
    if (!n) { *all_ok = 1; return ZKP_OK; }
    const void* field[6] = {pk, inf_pk, grp_off, sig, inf_sig, rand};
    const size_t bytes[6] = {n * 96, n, (m + 1) * 8, n * 192, n, n * 16};
    size_t off[6], total = 0;
    for (int i = 0; i < 6; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, m, dst, dst_len, &dm, &dof, &dd);
    char* dev = (char*)io.slot(3, total);
    const void* d[6];
    for (int i = 0; i < 6; i++) d[i] = io.put(dev + off[i], field[i], bytes[i]);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)d[0], n * 2)) || (rc = validate_dev(c, (const uint64_t*)d[3], n * 4)) ||
        (rc = zkp::grp_verify_dev(c, d[0], d[1], d[2], dm, dof, m, dd, dst_len, d[3], d[4], n, d[5], flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

int zkp_bls_fast_aggregate_verify_grouped_batch_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off,
                                                    const void* grp_off, const void* msgs, const void* offsets, size_t m, const void* dst, size_t dst_len,
                                                    const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, void* all_ok, void* stream) {
    if (grp_fav_args_bad(c, table, n_table, idx, n_idx, seg_off, grp_off, msgs, offsets, m, dst, dst_len, sig, n, rand, flags, all_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int rc;
    if ((rc = validate_on_stream(c, table, n_table * 2, S(stream))) || (rc = validate_on_stream(c, sig, n * 4, S(stream)))) return rc;
    return zkp::grp_fast_aggregate_verify_dev(c, table, n_table, idx, n_idx, seg_off, grp_off, msgs, offsets, m, dst, dst_len, sig, inf_sig, n, rand, flags,
                                              (int*)all_ok, S(stream));
}
// the seven arrays one after the other in slot 3 (256-byte aligned), the messages in slots 0..2, then the same driver
int zkp_bls_fast_aggregate_verify_grouped_batch(zkp_ctx* c, const uint64_t* table, size_t n_table, const uint32_t* idx, size_t n_idx, const uint64_t* seg_off,
                                                const uint64_t* grp_off, const uint8_t* msgs, const uint64_t* offsets, size_t m, const uint8_t* dst,
                                                size_t dst_len, const uint64_t* sig, const uint8_t* inf_sig, size_t n, const uint64_t* rand, int flags,
                                                int* all_ok) {
    if (grp_fav_args_bad(c, table, n_table, idx, n_idx, seg_off, grp_off, msgs, offsets, m, dst, dst_len, sig, n, rand, flags, all_ok) ||
        offsets_malformed(msgs, offsets, m))
        return ZKP_ERR_ARG;
    if ((n || n_idx) && (zkp::agg::offsets_malformed(seg_off, n, n_idx) || zkp::agg::rows_out_of_range(idx, n_idx, n_table))) return ZKP_ERR_ARG;
    if (grp_off && zkp::grp::offsets_malformed(grp_off, m, n)) return ZKP_ERR_ARG;
    if (!n) { *all_ok = 1; return ZKP_OK; }
    const void* field[7] = {table, idx, seg_off, grp_off, sig, inf_sig, rand};
    const size_t bytes[7] = {n_table * 96, n_idx * 4, (n + 1) * 8, (m + 1) * 8, n * 192, n, n * 16};
    size_t off[7], total = 0;
    for (int i = 0; i < 7; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, m, dst, dst_len, &dm, &dof, &dd);
    char* dev = (char*)io.slot(3, total);
    const void* d[7];
    for (int i = 0; i < 7; i++) d[i] = io.put(dev + off[i], field[i], bytes[i]);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)d[0], n_table * 2)) || (rc = validate_dev(c, (const uint64_t*)d[4], n * 4)) ||
        (rc = zkp::grp_fast_aggregate_verify_dev(c, d[0], n_table, d[1], n_idx, d[2], d[3], dm, dof, m, dd, dst_len, d[4], d[5], n, d[6], flags, c->d_flag + 1,
                                                 c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- hash-to-G1 and the min-sig BLS batch verifiers (zkp_bls_minsig.hip,
// include/zkp_bls_minsig.h)
extern "C" {

int zkp_hash_to_field_g1_batch_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out_u, void* stream) {
    if (h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || (n && !out_u)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return zkp::g1h_field_dev(c, msgs, offsets, n, dst, dst_len, out_u, S(stream));
}
int zkp_hash_to_field_g1_batch(zkp_ctx* c, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len, uint64_t* out_u) {
    if (h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || (n && !out_u) || offsets_malformed(msgs, offsets, n)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n, dst, dst_len, &dm, &dof, &dd);
    void* dout = io.out(4, out_u, n * 96);
    int rc;
    if ((rc = io.status()) || (rc = zkp::g1h_field_dev(c, dm, dof, n, dd, dst_len, dout, c->stream))) return rc;
    return io.finish();
}

int zkp_g1_map_from_fields_batch_dev(zkp_ctx* c, const void* u, size_t n, void* out, void* out_inf, void* stream) {
    if (!c || n > zkp::bls::MAX_N || (n && (!u || !out || !out_inf))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, u, n * 2, S(stream))) return rc;
    return zkp::g1h_map_dev(c, u, n, out, out_inf, S(stream));
}
int zkp_g1_map_from_fields_batch(zkp_ctx* c, const uint64_t* u, size_t n, uint64_t* out, uint8_t* out_inf) {
    if (!c || n > zkp::bls::MAX_N || (n && (!u || !out || !out_inf))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const void* du = io.in(0, u, n * 96);
    void* dout = io.out(4, out, n * 96);
    void* dinf = io.out(6, out_inf, n);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)du, n * 2)) || (rc = zkp::g1h_map_dev(c, du, n, dout, dinf, c->stream))) return rc;
    return io.finish();
}

int zkp_g1_clear_cofactor_batch_dev(zkp_ctx* c, const void* pts, const void* inf, size_t n, void* out, void* out_inf, void* stream) {
    if (!c || n > zkp::bls::MAX_N || (n && (!pts || !out || !out_inf))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, pts, n * 2, S(stream))) return rc;
    return zkp::g1h_clear_dev(c, pts, inf, n, out, out_inf, S(stream));
}
int zkp_g1_clear_cofactor_batch(zkp_ctx* c, const uint64_t* pts, const uint8_t* inf, size_t n, uint64_t* out, uint8_t* out_inf) {
    if (!c || n > zkp::bls::MAX_N || (n && (!pts || !out || !out_inf))) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const void* dp = io.in(0, pts, n * 96);
    const void* di = io.in(2, inf, n);
    void* dout = io.out(4, out, n * 96);
    void* dinf = io.out(6, out_inf, n);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)dp, n * 2)) || (rc = zkp::g1h_clear_dev(c, dp, di, n, dout, dinf, c->stream))) return rc;
    return io.finish();
}

int zkp_hash_to_g1_batch_dev(zkp_ctx* c, const void* msgs, const void* offsets, size_t n, const void* dst, size_t dst_len, void* out, void* out_inf,
                             void* stream) {
    if (h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || (n && (!out || !out_inf))) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    return zkp::g1h_hash_dev(c, msgs, offsets, n, dst, dst_len, out, out_inf, S(stream));
}
int zkp_hash_to_g1_batch(zkp_ctx* c, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len, uint64_t* out,
                         uint8_t* out_inf) {
    if (h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || (n && (!out || !out_inf)) || offsets_malformed(msgs, offsets, n)) return ZKP_ERR_ARG;
    if (!n) return ZKP_OK;
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n, dst, dst_len, &dm, &dof, &dd);
    void* dout = io.out(4, out, n * 96);
    void* dinf = io.out(6, out_inf, n);
    int rc;
    if ((rc = io.status()) || (rc = zkp::g1h_hash_dev(c, dm, dof, n, dd, dst_len, dout, dinf, c->stream))) return rc;
    return io.finish();
}

// k free pairs and s2 columns as the verifier hands them to the driver: (1, 1) for the general one, (0, 2) for the same-key one
static bool minsig_args_bad(const zkp_ctx* c, const void* pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig, size_t n,
                            const void* rand, int flags, const void* all_ok, size_t k, size_t s2, bool pk_always) {
    return h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || !all_ok || (flags & ~ZKP_BLS_POINTS_CHECKED) || n > zkp::bls::MAX_VERIFY_N ||
           zkp::rlc::args_bad(n, k, 0, s2) || ((n || pk_always) && !pk) || (n && (!sig || !rand));
}
int zkp_bls_minsig_verify_batch_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len,
                                    const void* sig, const void* inf_sig, size_t n, const void* rand, int flags, void* all_ok, void* stream) {
    if (minsig_args_bad(c, pk, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok, 1, 1, false)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int rc;
    if ((rc = validate_on_stream(c, pk, n * 4, S(stream))) || (rc = validate_on_stream(c, sig, n * 2, S(stream)))) return rc;
    return zkp::minsig_verify_dev(c, pk, inf_pk, msgs, offsets, dst, dst_len, sig, inf_sig, n, rand, flags, (int*)all_ok, S(stream));
}
// the arrays of points one after the other in slot 3 (256-byte aligned), the messages in slots 0..2, then the same driver
int zkp_bls_minsig_verify_batch(zkp_ctx* c, const uint64_t* pk, const uint8_t* inf_pk, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst,
                                size_t dst_len, const uint64_t* sig, const uint8_t* inf_sig, size_t n, const uint64_t* rand, int flags, int* all_ok) {
    if (minsig_args_bad(c, pk, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok, 1, 1, false) || offsets_malformed(msgs, offsets, n)) return ZKP_ERR_ARG;
    if (!n) { *all_ok = 1; return ZKP_OK; }
    const void* field[5] = {pk, inf_pk, sig, inf_sig, rand};
    const size_t bytes[5] = {n * 192, n, n * 96, n, n * 16};
    size_t off[5], total = 0;
    for (int i = 0; i < 5; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n, dst, dst_len, &dm, &dof, &dd);
    char* dev = (char*)io.slot(3, total);
    const void* d[5];
    for (int i = 0; i < 5; i++) d[i] = io.put(dev + off[i], field[i], bytes[i]);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)d[0], n * 4)) || (rc = validate_dev(c, (const uint64_t*)d[2], n * 2)) ||
        (rc = zkp::minsig_verify_dev(c, d[0], d[1], dm, dof, dd, dst_len, d[2], d[3], n, d[4], flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

int zkp_bls_minsig_verify_samekey_batch_dev(zkp_ctx* c, const void* pk, const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig,
                                            const void* inf_sig, size_t n, const void* rand, int flags, void* all_ok, void* stream) {
    if (minsig_args_bad(c, pk, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok, 0, n ? 2 : 0, true)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int rc;
    if ((rc = validate_on_stream(c, pk, 4, S(stream))) || (rc = validate_on_stream(c, sig, n * 2, S(stream)))) return rc;
    return zkp::minsig_verify_samekey_dev(c, pk, msgs, offsets, dst, dst_len, sig, inf_sig, n, rand, flags, (int*)all_ok, S(stream));
}
int zkp_bls_minsig_verify_samekey_batch(zkp_ctx* c, const uint64_t* pk, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                                        const uint64_t* sig, const uint8_t* inf_sig, size_t n, const uint64_t* rand, int flags, int* all_ok) {
    if (minsig_args_bad(c, pk, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok, 0, n ? 2 : 0, true) || offsets_malformed(msgs, offsets, n))
        return ZKP_ERR_ARG;
    if (!n) { *all_ok = 1; return ZKP_OK; }
    const void* field[4] = {pk, sig, inf_sig, rand};
    const size_t bytes[4] = {192, n * 96, n, n * 16};
    size_t off[4], total = 0;
    for (int i = 0; i < 4; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n, dst, dst_len, &dm, &dof, &dd);
    char* dev = (char*)io.slot(3, total);
    const void* d[4];
    for (int i = 0; i < 4; i++) d[i] = io.put(dev + off[i], field[i], bytes[i]);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)d[0], 4)) || (rc = validate_dev(c, (const uint64_t*)d[1], n * 2)) ||
        (rc = zkp::minsig_verify_samekey_dev(c, d[0], dm, dof, dd, dst_len, d[1], d[2], n, d[3], flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- G2 segment sums, the min-sig FastAggregateVerify and AggregateVerify
// (zkp_bls_agg_g2.hip, include/zkp_bls_agg_g2.h)
namespace {
bool agg2_sum_args_bad(const zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, const void* out,
                       const void* out_inf, const void* status) {
    return !c || zkp::agg2::args_bad(n_table, n_idx, n_seg) || (n_table && !table) || (n_idx && !idx) || ((n_seg || n_idx) && !seg_off) ||
           (n_seg && (!out || !out_inf || !status));
}
bool agg2_minsig_args_bad(const zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, const void* msgs,
                          const void* offsets, const void* dst, size_t dst_len, const void* sig, size_t n, const void* rand, int flags, const void* all_ok) {
    return h2c_msgs_bad(c, msgs, offsets, n, dst, dst_len) || !all_ok || (flags & ~ZKP_BLS_POINTS_CHECKED) || n > zkp::bls::MAX_VERIFY_N ||
           zkp::rlc::args_bad(n, 1, 0, 1) || (n && (!sig || !rand)) || zkp::agg2::args_bad(n_table, n_idx, n) || (n_table && !table) || (n_idx && !idx) ||
           ((n || n_idx) && !seg_off);
}
bool aggv_args_bad(const zkp_ctx* c, const void* pk, const void* msgs, const void* offsets, size_t n_msg, const void* seg_off, const void* dst, size_t dst_len,
                   const void* sig, size_t n, const void* rand, int flags, const void* all_ok) {
    // zkp_bls_verify_batch's refusals on n_msg, but sig and rand hold n rows: with messages and no signature (malformed) they may be null
    return h2c_msgs_bad(c, msgs, offsets, n_msg, dst, dst_len) || !all_ok || (flags & ~ZKP_BLS_POINTS_CHECKED) || zkp::rlc::args_bad(n_msg, 1, 1, 0) ||
           zkp::agg2::verify_args_bad(n_msg, n) || (n_msg && !pk) || (n && (!sig || !rand)) || ((n || n_msg) && !seg_off);
}
}  // namespace

extern "C" {

int zkp_g2_segment_sum_batch_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off, size_t n_seg, void* out,
                                 void* out_inf, void* status, void* stream) {
    if (agg2_sum_args_bad(c, table, n_table, idx, n_idx, seg_off, n_seg, out, out_inf, status)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    if (int rc = validate_on_stream(c, table, n_table * 4, S(stream))) return rc;
    return zkp::agg2_segment_sum_dev(c, table, n_table, idx, n_idx, seg_off, n_seg, out, out_inf, status, S(stream));
}
int zkp_g2_segment_sum_batch(zkp_ctx* c, const uint64_t* table, size_t n_table, const uint32_t* idx, size_t n_idx, const uint64_t* seg_off, size_t n_seg,
                             uint64_t* out, uint8_t* out_inf, uint8_t* status) {
    if (agg2_sum_args_bad(c, table, n_table, idx, n_idx, seg_off, n_seg, out, out_inf, status)) return ZKP_ERR_ARG;
    if (!n_seg && !n_idx) return ZKP_OK;
    if (zkp::agg::offsets_malformed(seg_off, n_seg, n_idx) || zkp::agg::rows_out_of_range(idx, n_idx, n_table)) return ZKP_ERR_ARG;
    HostIO io(c);
    const void* dt = io.in(0, table, n_table * 192);
    const void* di = io.in(1, idx, n_idx * 4);
    const void* ds = io.in(2, seg_off, (n_seg + 1) * 8);
    void* dout = io.out(4, out, n_seg * 192);
    void* dinf = io.out(5, out_inf, n_seg);
    void* dst = io.out(6, status, n_seg);
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)dt, n_table * 4)) ||
        (rc = zkp::agg2_segment_sum_dev(c, dt, n_table, di, n_idx, ds, n_seg, dout, dinf, dst, c->stream)))
        return rc;
    return io.finish();
}

int zkp_bls_minsig_fast_aggregate_verify_batch_dev(zkp_ctx* c, const void* table, size_t n_table, const void* idx, size_t n_idx, const void* seg_off,
                                                   const void* msgs, const void* offsets, const void* dst, size_t dst_len, const void* sig,
                                                   const void* inf_sig, size_t n, const void* rand, int flags, void* all_ok, void* stream) {
    if (agg2_minsig_args_bad(c, table, n_table, idx, n_idx, seg_off, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int rc;
    if ((rc = validate_on_stream(c, table, n_table * 4, S(stream))) || (rc = validate_on_stream(c, sig, n * 2, S(stream)))) return rc;
    return zkp::agg2_minsig_verify_dev(c, table, n_table, idx, n_idx, seg_off, msgs, offsets, dst, dst_len, sig, inf_sig, n, rand, flags, (int*)all_ok,
                                       S(stream));
}
// the six arrays one after the other in slot 3 (256-byte aligned), the messages in slots 0..2, then the same driver
int zkp_bls_minsig_fast_aggregate_verify_batch(zkp_ctx* c, const uint64_t* table, size_t n_table, const uint32_t* idx, size_t n_idx, const uint64_t* seg_off,
                                               const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len, const uint64_t* sig,
                                               const uint8_t* inf_sig, size_t n, const uint64_t* rand, int flags, int* all_ok) {
    if (agg2_minsig_args_bad(c, table, n_table, idx, n_idx, seg_off, msgs, offsets, dst, dst_len, sig, n, rand, flags, all_ok) ||
        offsets_malformed(msgs, offsets, n))
        return ZKP_ERR_ARG;
    if ((n || n_idx) && (zkp::agg::offsets_malformed(seg_off, n, n_idx) || zkp::agg::rows_out_of_range(idx, n_idx, n_table))) return ZKP_ERR_ARG;
    if (!n) { *all_ok = 1; return ZKP_OK; }
    const void* field[6] = {table, idx, seg_off, sig, inf_sig, rand};
    const size_t bytes[6] = {n_table * 192, n_idx * 4, (n + 1) * 8, n * 96, n, n * 16};
    size_t off[6], total = 0;
    for (int i = 0; i < 6; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n, dst, dst_len, &dm, &dof, &dd);
    char* dev = (char*)io.slot(3, total);
    const void* d[6];
    for (int i = 0; i < 6; i++) d[i] = io.put(dev + off[i], field[i], bytes[i]);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)d[0], n_table * 4)) || (rc = validate_dev(c, (const uint64_t*)d[3], n * 2)) ||
        (rc = zkp::agg2_minsig_verify_dev(c, d[0], n_table, d[1], n_idx, d[2], dm, dof, dd, dst_len, d[3], d[4], n, d[5], flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

int zkp_bls_aggregate_verify_batch_dev(zkp_ctx* c, const void* pk, const void* inf_pk, const void* msgs, const void* offsets, size_t n_msg, const void* seg_off,
                                       const void* dst, size_t dst_len, const void* sig, const void* inf_sig, size_t n, const void* rand, int flags,
                                       void* all_ok, void* stream) {
    if (aggv_args_bad(c, pk, msgs, offsets, n_msg, seg_off, dst, dst_len, sig, n, rand, flags, all_ok)) return ZKP_ERR_ARG;
    DEV_ENTER(c, stream);
    int rc;
    if ((rc = validate_on_stream(c, pk, n_msg * 2, S(stream))) || (rc = validate_on_stream(c, sig, n * 4, S(stream)))) return rc;
    return zkp::aggv_verify_dev(c, pk, inf_pk, msgs, offsets, n_msg, seg_off, dst, dst_len, sig, inf_sig, n, rand, flags, (int*)all_ok, S(stream));
}
// the six arrays one after the other in slot 3 (256-byte aligned), the messages in slots 0..2, then the same driver
int zkp_bls_aggregate_verify_batch(zkp_ctx* c, const uint64_t* pk, const uint8_t* inf_pk, const uint8_t* msgs, const uint64_t* offsets, size_t n_msg,
                                   const uint64_t* seg_off, const uint8_t* dst, size_t dst_len, const uint64_t* sig, const uint8_t* inf_sig, size_t n,
                                   const uint64_t* rand, int flags, int* all_ok) {
    if (aggv_args_bad(c, pk, msgs, offsets, n_msg, seg_off, dst, dst_len, sig, n, rand, flags, all_ok) || offsets_malformed(msgs, offsets, n_msg))
        return ZKP_ERR_ARG;
    if ((n || n_msg) && zkp::agg::offsets_malformed(seg_off, n, n_msg)) return ZKP_ERR_ARG;
    if (!n_msg) { *all_ok = n ? 0 : 1; return ZKP_OK; }                   // no message: no signature holds, every segment is empty
    const void* field[6] = {pk, inf_pk, seg_off, sig, inf_sig, rand};
    const size_t bytes[6] = {n_msg * 96, n_msg, (n + 1) * 8, n * 192, n, n * 16};
    size_t off[6], total = 0;
    for (int i = 0; i < 6; i++) {
        off[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    HostIO io(c);
    const uint8_t* dm;
    const void *dof, *dd;
    stage_msgs(io, 0, 1, 2, msgs, offsets, n_msg, dst, dst_len, &dm, &dof, &dd);
    char* dev = (char*)io.slot(3, total);
    const void* d[6];
    for (int i = 0; i < 6; i++) d[i] = io.put(dev + off[i], field[i], bytes[i]);
    io.get(all_ok, c->d_flag + 1, sizeof(int));
    int rc;
    if ((rc = io.status()) || (rc = validate_dev(c, (const uint64_t*)d[0], n_msg * 2)) || (rc = validate_dev(c, (const uint64_t*)d[3], n * 4)) ||
        (rc = zkp::aggv_verify_dev(c, d[0], d[1], dm, dof, n_msg, d[2], dd, dst_len, d[3], d[4], n, d[5], flags, c->d_flag + 1, c->stream)))
        return rc;
    return io.finish();
}

}  // extern "C"
