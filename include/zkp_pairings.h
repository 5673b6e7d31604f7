/*
 * include/zkp_pairings.h -- C ABI of libzkp_pairings.so, the MI355X (gfx950) batched BLS12-381
 * pairing engine.  This is the drop-in boundary for the pairing-check path of
 * 0xWOLAND/zkvm-pairings: a Rust/cgo/ctypes binding declares exactly these symbols
 * (see INTEGRATION.md for the Rust `extern "C"` block).
 *
 * Reference interface each entry point stands in for (paths relative to /root/reference):
 *   zkp_pairing_batch               pairing(&G1Affine,&G2Affine)->Gt        src/pairings.rs (declared at
 *   zkp_multi_miller_loop_batch     multi_miller_loop(&[(G1,G2)])            src/lib.rs:12; the file is EMPTY in
 *   zkp_final_exponentiation_batch  MillerLoopResult::final_exponentiation   this snapshot - semantics defined in
 *   zkp_pairing_check_batch         pairing(..) == Gt::identity()            SURVEY.md S6 / DESIGN.md)
 *   zkp_gt_identity                 Gt::identity() == Fp12::one()            src/fp12.rs:87-89
 *   zkp_g1_is_valid_batch           G1Affine::is_valid                       src/g1.rs:49-62  (is_on_curve :95-101,
 *                                                                            is_torsion_free :111-115)
 *   zkp_g2_is_valid_batch           G2Affine::is_valid                       src/g2.rs:57-69  (:109-120, :166-170)
 *   zkp_g1_mul_batch / g2           &G1Affine * &Fr / &G2Affine * &Fr         src/g1.rs:130-153 (bit-0 bug F5 NOT
 *                                                                            mirrored), src/g2.rs:185-208
 *   zkp_g1_add_batch / g2           G1Affine + G1Affine / G2Affine + G2Affine src/g1.rs:155-187, src/g2.rs:210-242 (P + (-P): F7)
 *   zkp_g1_msm_batch / g2           sum_i [k_i] P_i (no upstream counterpart: Add and Mul composed)
 *   zkp_fp_op_batch                 bls12381_sys_bigint(out, op, a, b)       src/fp.rs:376,443 (op 0 = mul, 1 = add); also
 *                                   Fp::sub / neg / square / invert          src/fp.rs:307-319, 383-411, 453-455
 *   zkp_fr_op_batch                 Fr add / sub / neg / mul / square / invert src/fr.rs:402-411, 384-398, 415-431, 365-381, 225-227, 266-362
 *   zkp_fr_from_wide_batch          Fr::from_bytes_wide / from_u512           src/fr.rs:192-217
 *   zkp_fr_fold_batch,              sum_c w_c x_{c,i} in Fr and the batched Groth16 verifier built on it (no upstream counterpart:
 *   zkp_groth16_verify_batch        Fr Mul / Add and pairing() composed)
 *   zkp_fr_invert_batch             Fr::invert over a batch by Montgomery's trick (one power per CALL) src/fr.rs:266-362
 *   zkp_fr_eval_batch,              a polynomial in evaluation form at a point (barycentric formula over the 2^k-th roots of unity,
 *   zkp_kzg_verify_batch            FR_GENERATOR / FR_S of src/common.rs) and the batch KZG opening verifier (no upstream counterpart)
 *   zkp_tower_op_batch              Fp2 / Fp6 / Fp12 mul, square, mul_by_014, src/fp2.rs:171-209, src/fp6.rs:188-288,
 *                                   conjugate, frobenius_map (the TRUE map),  src/fp12.rs:99-210 (:143-170 is wrong)
 *                                   invert, mul_by_nonresidue, mul_by_1 / 01  src/fp2.rs:95-102,161-168,278-296, src/fp6.rs:102-141,291-309
 *   zkp_points_check_batch          raw points -> Fp::from_bytes, is_valid, pairing check in one call  src/fp.rs:165-207, src/g1.rs:49-62, src/g2.rs:57-69
 *   zkp_fp_sqrt_batch / fp2         Fp::sqrt, Fp2::sqrt                      src/fp.rs:280-300, src/fp2.rs:231-273
 *   zkp_g*_(de)compress_batch,      compressed points (48 / 96 B): decompression = x^3 + b, a square root, the sort flag's sign;
 *   zkp_points_check_compressed_*   the points check on compressed inputs (see "compressed points" below)
 *   zkp_pairing_*_multi             the same pairing()/check over several GPUs from ONE host thread
 *   zkp_comm_*, zkp_*_allreduce     one rank per GPU: the check + the path's one RCCL collective
 *
 * Wire formats (all little-endian, canonical representatives in [0,p), identical to the
 * reference's in-memory structs):
 *   fp    uint64_t[6]                          Fp.0                         src/fp.rs:24
 *   fp2   c0 | c1                    (12 u64)  Fp2{c0,c1}                   src/fp2.rs:10-15
 *   fp12  c0.c0.c0, c0.c0.c1, c0.c1.c0 ... c1.c2.c1 (72 u64)                src/fp12.rs:13-16, src/fp6.rs:13-17
 *   g1    x | y                      (12 u64)  + parallel uint8 is_infinity src/g1.rs:7-11
 *   g2    x.c0 | x.c1 | y.c0 | y.c1  (24 u64)  + parallel uint8 is_infinity src/g2.rs:8-12
 *   fr    uint64_t[4] canonical scalar                                      src/fr.rs (Fr.0)
 *
 * Ownership: the caller owns every buffer it passes (host or device); the library owns the
 * workspace inside zkp_ctx.  Errors: 0 on success, negative zkp_status otherwise; the library never
 * aborts and never unwinds across this boundary (the reference's panics F7 become status bytes).
 * Inputs must be canonical (< p): non-canonical limbs give ZKP_ERR_NONCANONICAL when validation is on
 * (zkp_set_validate), unspecified field values otherwise.
 * Points: ONLY the infinity flag marks the identity - coordinates (0, 0) with the flag clear are a point like any other (EIP-197-style
 * callers must set the flag).  The pairing entry points do not validate points (zkp_points_check_batch and the RLC path do): on any
 * canonical input, on or off the curve, in or out of the prime-order subgroups, they compute exactly what is written below.
 * Threading: a zkp_ctx is bound to one GPU and is not thread-safe; use one ctx per thread / rank.  The *_dev calls
 * of one ctx may be issued on different streams: each call first makes its stream wait (an event, no host wait) for the
 * previous call's use of the context's workspace, so they never overlap on it.
 * There is NO CPU fallback: zkp_init fails with ZKP_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef ZKP_PAIRINGS_H
#define ZKP_PAIRINGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkp_ctx zkp_ctx;

typedef enum {
    ZKP_OK = 0,
    ZKP_ERR_ARG = -1,          /* null pointer / bad size */
    ZKP_ERR_NO_DEVICE = -2,    /* no usable HIP device */
    ZKP_ERR_HIP = -3,          /* a HIP runtime call failed; see zkp_last_error */
    ZKP_ERR_NONCANONICAL = -4, /* an input limb array is >= p (validation mode) */
    ZKP_ERR_OOM = -5,
    ZKP_ERR_COMM = -6          /* an RCCL call failed or the context has no communicator; see zkp_last_error */
} zkp_status;

/* zkp_fp_op_batch: the operation in bits 0..3, the limb core in bit 4.  0 and 1 are the op numbers of the zkVM precompile
 * bls12381_sys_bigint (src/fp.rs:376,443); unary operations ignore b (may be NULL). */
typedef enum {
    ZKP_FP_MUL = 0,
    ZKP_FP_ADD = 1,
    ZKP_FP_SUB = 2,
    ZKP_FP_NEG = 3,
    ZKP_FP_SQUARE = 4,
    ZKP_FP_INVERT = 5,      /* 0 gives 0 (the reference returns None, src/fp.rs:307-319) */
    ZKP_FP_CORE28 = 16      /* OR-ed in: run on the 14 x 28-bit carry-free core of the cooperative family instead of
                               the 12 x 32-bit Montgomery core */
} zkp_fp_op;

/* zkp_tower_op_batch: one tower operation per 72-u64 record.  Smaller tower elements occupy the leading coefficients
 * of a record (Fp2: 12 u64, Fp6: 36 u64); the rest of an input must be zero and the rest of the result is zero. */
typedef enum {
    ZKP_TOWER_FP2_MUL = 0,
    ZKP_TOWER_FP2_SQUARE = 1,
    ZKP_TOWER_FP6_MUL = 2,
    ZKP_TOWER_FP6_SQUARE = 3,
    ZKP_TOWER_FP6_FROBENIUS = 4,            /* x^p (NOT what src/fp6.rs:142-176 computes) */
    ZKP_TOWER_FP12_MUL = 5,
    ZKP_TOWER_FP12_SQUARE = 6,
    ZKP_TOWER_FP12_MUL_BY_014 = 7,          /* b = c0 | c1 | c4 (three Fp2) in the first 36 u64 of its record */
    ZKP_TOWER_FP12_FROBENIUS = 8,           /* x^p */
    ZKP_TOWER_FP12_CONJUGATE = 9,
    ZKP_TOWER_FP12_CYCLOTOMIC_SQUARE = 10,  /* Granger-Scott; input in the cyclotomic subgroup */
    ZKP_TOWER_FP12_CYCLOTOMIC_POW2K = 11,   /* g^(2^repeat), 1 <= repeat <= 64: compressed squarings + decompression
                                               (the building block of the final exponentiation's x-power chains) */
    ZKP_TOWER_FP12_CYCLOTOMIC_DECOMPRESS = 12, /* Karabina decompression: c0.c0 and c1.c1 of the result are recomputed from
                                               the other four Fp2 coefficients of the record (cooperative family only) */
    /* the rest of the tower functions SURVEY.md 8(a) names, as direct hooks.  The inversions return the ZERO record for a
     * non-invertible (zero) input, where the reference returns None. */
    ZKP_TOWER_FP2_INVERT = 13,              /* src/fp2.rs:278-296 */
    ZKP_TOWER_FP2_MUL_BY_NONRESIDUE = 14,   /* (c0 - c1) + (c0 + c1) u, src/fp2.rs:161-168 */
    ZKP_TOWER_FP2_MUL_FP = 15,              /* Mul<&Fp> for Fp2, src/fp2.rs:95-102: b = the Fp value in the first 6 u64 of its record */
    ZKP_TOWER_FP6_MUL_BY_1 = 16,            /* src/fp6.rs:102-108: b = c1 (Fp2) in the first 12 u64 */
    ZKP_TOWER_FP6_MUL_BY_01 = 17,           /* src/fp6.rs:110-127: b = c0 | c1 in the first 24 u64 */
    ZKP_TOWER_FP6_MUL_BY_NONRESIDUE = 18,   /* * v, src/fp6.rs:130-141 */
    ZKP_TOWER_FP6_INVERT = 19,              /* src/fp6.rs:291-309 */
    ZKP_TOWER_FP12_INVERT = 20              /* src/fp12.rs:186-190 */
} zkp_tower_op;

/* which Miller-loop/final-exp kernel family the context uses */
typedef enum {
    ZKP_KERNEL_AUTO = 0,
    ZKP_KERNEL_THREAD = 1,  /* one pairing per lane, 12x32-bit Montgomery limbs */
    ZKP_KERNEL_COOP = 2     /* lane-group-cooperative, LDS-staged tower (hot path) */
} zkp_kernel_kind;

int zkp_abi_version(void);
const char* zkp_strerror(int status);

/* device = HIP device ordinal of this process (LOCAL_RANK under torchrun). */
int zkp_init(int device, zkp_ctx** out_ctx);
void zkp_free(zkp_ctx* ctx);
const char* zkp_last_error(const zkp_ctx* ctx);
int zkp_set_validate(zkp_ctx* ctx, int on);
int zkp_set_kernel(zkp_ctx* ctx, int kind /* zkp_kernel_kind */);
int zkp_device_info(const zkp_ctx* ctx, int* cus, int* clock_khz, char* name, size_t name_len);

/* Gt::identity(): 72 u64, c0.c0.c0 = 1, rest 0. */
const uint64_t* zkp_gt_identity(void);

/* ---- host-pointer entry points (H2D copy, kernels, D2H copy, synchronous) ---------------------- */
/* out_gt[i] = pairing(g1[i], g2[i]); inf1/inf2 may be NULL (= no infinities).  Every pairing-shaped entry point (pairing, check, product
 * check, their _dev and _multi flavours, both kernel families) returns exactly final_exponentiation(multi_miller_loop(..)) of the
 * upstream-shaped Miller loop (ePrint 2010/354 Alg. 26 / 27) for ANY canonical input; a pair with an infinity flag contributes one. */
int zkp_pairing_batch(zkp_ctx* ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2,
                      size_t n, uint64_t* out_gt);
/* n_checks groups of k consecutive pairs; out_ml[c] = multi_miller_loop(group c) (72 u64 each). */
int zkp_multi_miller_loop_batch(zkp_ctx* ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1,
                                const uint8_t* inf2, size_t n_checks, size_t k, uint64_t* out_ml);
/* f^(3 (p^12 - 1) / r); f = 0 (a Miller loop on points off the curves can give it, e.g. an unflagged (0, 0) G2 point) gives the ZERO
 * record, never Gt::identity(), so a check or product check whose Miller value is zero fails (ok = 0, all_ok = 0, is_one = 0) where the
 * reference panics in Fp12::invert().unwrap() (F7). */
int zkp_final_exponentiation_batch(zkp_ctx* ctx, const uint64_t* f, size_t n, uint64_t* out_gt);
/* ok[c] = (final_exponentiation(multi_miller_loop(group c)) == Gt::identity()); ok may be NULL.
 * *all_ok = AND over this call's checks (the cross-GPU AND is the caller's single RCCL all-reduce). */
int zkp_pairing_check_batch(zkp_ctx* ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1,
                            const uint8_t* inf2, size_t n_checks, size_t k, uint8_t* ok, int* all_ok);
/* ---- the whole batch as ONE product check (SURVEY.md 8e variant; BLS batch verification shape) ----
 * multi_miller_loop(&[(P_0,Q_0) .. (P_n-1,Q_n-1)]) over ALL n pairs -> one Fp12 (72 u64); n == 0 gives one.
 * A multi-GPU host multiplies the per-GPU values (all-gather of 576 B per rank, zkp_fp12_product) and runs
 * ONE zkp_final_exponentiation_batch(n = 1). */
int zkp_miller_product(zkp_ctx* ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2,
                       size_t n, uint64_t* out_ml);
/* out = f_0 * f_1 * ... * f_n-1 (Fp12 Mul, reference src/fp12.rs:193-210, folded by a log-depth tree); n == 0 gives one. */
int zkp_fp12_product(zkp_ctx* ctx, const uint64_t* f, size_t n, uint64_t* out);
/* *is_one = (final_exponentiation(zkp_miller_product(..)) == Gt::identity()); out_gt (72 u64) may be NULL. */
int zkp_pairing_product_check(zkp_ctx* ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1,
                              const uint8_t* inf2, size_t n, uint64_t* out_gt, int* is_one);
/* status[i]: 0 valid (or infinity), 1 not on curve, 2 not torsion free. */
int zkp_g1_is_valid_batch(zkp_ctx* ctx, const uint64_t* g1, const uint8_t* inf, size_t n, uint8_t* status);
int zkp_g2_is_valid_batch(zkp_ctx* ctx, const uint64_t* g2, const uint8_t* inf, size_t n, uint8_t* status);
/* out[i] = [k_i] p_i (affine); base_stride 0 broadcasts one base point. out_inf may be NULL. */
int zkp_g1_mul_batch(zkp_ctx* ctx, const uint64_t* base, size_t base_stride, const uint64_t* scalars, size_t n,
                     uint64_t* out, uint8_t* out_inf);
int zkp_g2_mul_batch(zkp_ctx* ctx, const uint64_t* base, size_t base_stride, const uint64_t* scalars, size_t n,
                     uint64_t* out, uint8_t* out_inf);
/* ---- group addition and multi-scalar multiplication (on the 14 x 28-bit core whatever zkp_set_kernel says) --------------------------
 * out[i] = a[i] + b[i] (G1Affine / G2Affine Add, src/g1.rs:155-187, src/g2.rs:210-242); inf_a / inf_b / out_inf may be NULL (no infinities /
 * not wanted).  An infinite result is written as (0, 1) with out_inf = 1, as zkp_g*_mul_batch does.  Finite results equal the reference's
 * bit for bit.  F7 divergence: P + (-P) gives the identity; the reference's affine Add panics there (it inverts x_Q - x_P = 0).
 * MSM: n_msm independent sums out[j] = sum_{i<m} [k_{j,i}] P_{j,i}.  Scalars are full 256-bit integers, 4 u64 each, row j of m scalars
 * per sum (same contract as zkp_g1_mul_batch: no reduction mod r, no dropped bit 0).  shared_bases != 0: every sum uses the same m points
 * (points / inf hold m entries), else m * n_msm.  m * n_msm <= 2^24 and m >= 1 (when n_msm > 0), else ZKP_ERR_ARG.  Bucket method: c-bit
 * signed windows (c from 2 to 16, chosen from m), a radix sort of the digits, load-balanced bucket sums, one inversion per sum.
 * Workspace (grow-only, owned by the context, layout zkvm_pairings_amd/csrc/zkp_msm_plan.hpp): per pass 16 B per digit key
 * (W = 256/c + 1 keys per term), the converted points (128 B per G1 / 256 B per G2 point), W (192 B G1 / 384 B G2) / 16 B of partial sums per
 * term, and W 2^(c-1) buckets of 192 / 384 B per sum.  For example about 1.0 KB per term for a G1 MSM of 2^20 terms (c = 16),
 * 1.6 KB for G2. */
int zkp_g1_add_batch(zkp_ctx* ctx, const uint64_t* a, const uint8_t* inf_a, const uint64_t* b, const uint8_t* inf_b, size_t n, uint64_t* out,
                     uint8_t* out_inf);
int zkp_g2_add_batch(zkp_ctx* ctx, const uint64_t* a, const uint8_t* inf_a, const uint64_t* b, const uint8_t* inf_b, size_t n, uint64_t* out,
                     uint8_t* out_inf);
int zkp_g1_msm_batch(zkp_ctx* ctx, const uint64_t* points, const uint8_t* inf, const uint64_t* scalars, size_t m, size_t n_msm, int shared_bases,
                     uint64_t* out, uint8_t* out_inf);
int zkp_g2_msm_batch(zkp_ctx* ctx, const uint64_t* points, const uint8_t* inf, const uint64_t* scalars, size_t m, size_t n_msm, int shared_bases,
                     uint64_t* out, uint8_t* out_inf);
/* ---- batch verification by random linear combination (RLC) ------------------------------------------------------------------------
 * zkp_g1_mul_endo_batch: out[i] = [a_i] P_i + [b_i] (beta x_i, -y_i), ab = 2 u64 per point (a_i, b_i), on the 28-bit core whatever
 * zkp_set_kernel says; inf / out_inf may be NULL; an infinite result is (0, 1) with out_inf = 1.  For P in G1 (beta x, -y) = [z^2] P with
 * z = 0xd201000000010000, so the result equals [a_i + b_i z^2] P_i: a 128-bit multiple for 64 doublings.  Outside G1 it is still exactly
 * [a] P + [b] (beta x, -y).
 * zkp_pairing_check_batch_rlc: n_checks independent checks verified as ONE,
 *     *all_ok = ( prod_c ( prod_j e(P_cj, Q_cj) )^(r_c) == Gt::identity() )  AND every point valid AND no (a_c, b_c) = (0, 0),
 * r_c = a_c + b_c z^2 from rand[2c], rand[2c + 1] (draw them uniformly at random, per call, from a cryptographic source: a batch of
 * checks that do not all hold then passes with probability at most 2^-128 plus the chance of guessing rand).  Check c is the product of
 * its k free pairs (g1 / g2 / inf1 / inf2 laid out as zkp_pairing_check_batch), its s2 pairs (col_g1[c][j], fixed_g2[j]) and its s1 pairs
 * (fixed_g1[j], col_g2[c][j]) - col_* are n_checks x s rows (one row per check), fixed_* hold s points; every inf* may be NULL.  Expanded
 * into k + s1 + s2 pairs per check, it is exactly what zkp_pairing_check_batch tests: *all_ok = 1 implies (with the probability above)
 * that every check holds, and a batch of valid checks always gives 1.  Cost: N k endomorphism scalings + one Miller product over them, one
 * G1 MSM of n_checks terms per fixed-G2 column, one G2 MSM per fixed-G1 column, one Miller product over the s1 + s2 column pairs, ONE
 * final exponentiation.  RLC is sound for prime-order points only: unless flags has ZKP_RLC_POINTS_CHECKED every input point (fixed ones
 * included) goes through is_valid first.  Invalid points and zero scalars give *all_ok = 0, not an error.  n_checks == 0 gives 1; k == 0
 * needs s1 + s2 > 0.  ZKP_ERR_ARG: null pointers with nonzero counts, n_checks * k beyond zkp_pairing_check_batch's limits (n <= 2^31 - 1,
 * k <= 65535, n k <= 2^31 - 1), s1 or s2 > 65535, n_checks > 2^24 with any column, flags other than ZKP_RLC_POINTS_CHECKED.  Validation
 * mode covers every coordinate array.  The _dev flavour is asynchronous (no host read-back) and capturable into a hipGraph once the
 * context's workspaces have reached the call's size; d_all_ok (one int32) is required.
 * Workspace (grow-only, layout zkvm_pairings_amd/csrc/zkp_rlc_plan.hpp) per check: 97 B per free pair (scaled point + flag), 97 B per
 * fixed-G2 column and 193 B per fixed-G1 column (the column-major copy), 32 B of scalar per column (at most one copy per column), 2 B
 * per free pair and 1 B per column point of status without ZKP_RLC_POINTS_CHECKED; plus the MSM workspace of n_checks terms per column
 * (about 1.0 KB per G1 term and 1.6 KB per G2 term, see above) and, as for zkp_pairing_check_batch, the Miller loop's own workspace. */
typedef struct {
    size_t n_checks;
    size_t k;  const void *g1, *g2, *inf1, *inf2;                         /* k free pairs per check, laid out as zkp_pairing_check_batch */
    size_t s2; const void *col_g1, *col_inf1, *fixed_g2, *fixed_inf2;     /* s2 columns: one G1 per check (n_checks x s2, row per check), one fixed G2 each */
    size_t s1; const void *col_g2, *col_inf2, *fixed_g1, *fixed_inf1;     /* s1 columns: one G2 per check, one fixed G1 each */
} zkp_rlc_batch;
#define ZKP_RLC_POINTS_CHECKED 1   /* flags: skip the subgroup checks (caller guarantees every point is valid) */
int zkp_g1_mul_endo_batch(zkp_ctx* ctx, const uint64_t* base, const uint8_t* inf, const uint64_t* ab, size_t n, uint64_t* out, uint8_t* out_inf);
int zkp_g1_mul_endo_batch_dev(zkp_ctx* ctx, const void* d_base, const void* d_inf, const void* d_ab, size_t n, void* d_out, void* d_out_inf,
                              void* stream);
/* host flavour: the batch's pointers are host arrays */
int zkp_pairing_check_batch_rlc(zkp_ctx* ctx, const zkp_rlc_batch* b, const uint64_t* rand /* 2 u64 per check */, int flags, int* all_ok);
/* device flavour: the batch's pointers, d_rand and d_all_ok are device pointers (the descriptor itself is a host struct) */
int zkp_pairing_check_batch_rlc_dev(zkp_ctx* ctx, const zkp_rlc_batch* b, const void* d_rand, int flags, void* d_all_ok, void* stream);

/* ---- the scalar field Fr, the Fr fold and the batched Groth16 verifier (symbols added under ABI version 4) -----------------------------
 * Fr elements are 4 u64, little-endian, canonical (< r, the order of G1 / G2 / Gt), as the MSM and scalar-multiplication scalars.
 * zkp_fr_op_batch: out[i] = a[i] op b[i] (op: zkp_fr_op; unary operations ignore b, which may be NULL); 0 inverts to 0 where the
 * reference returns None (src/fr.rs:266-362).  Validation mode (zkp_set_validate): an element >= r gives ZKP_ERR_NONCANONICAL on the
 * host flavour; the _dev flavour ORs into the context's validation word (zkp_take_validation_status_dev) like every other _dev call.
 * zkp_fr_from_wide_batch: out[i] = the 512-bit little-endian integer bytes[64 i .. 64 i + 63] mod r (Fr::from_bytes_wide,
 * src/fr.rs:192-217); any input is legal.
 * zkp_fr_fold_batch: out[i] = sum_c w[c] x[c][i] mod r for i < l, and *sum_w = sum_c w[c] mod r (sum_w may be NULL); w holds n elements,
 * x n rows of l.  Inputs are canonical (validation mode as above); n <= 2^24, l <= 65535, n l <= 2^31 - 1, else ZKP_ERR_ARG; n == 0
 * gives zeros.  The sums are accumulated as exact integers (a product is below 2^512, 2^24 of them below 2^544 = 17 words) and
 * reduced once per output.  Workspace (grow-only, layout zkvm_pairings_amd/csrc/zkp_groth16_plan.hpp): 68 B per output and workgroup,
 * at most 1024 workgroups per tile of 64 outputs - 4.5 MB at worst.  The _dev flavours are asynchronous and capturable into a hipGraph
 * once that workspace has reached the call's size.
 * zkp_groth16_verify_batch: n Groth16 proofs (A_c, B_c, C_c) with n_inputs public inputs x_{c,i} each, against ONE verifying key.
 * Proof c is valid iff e(A_c, B_c) == e(alpha, beta) e(vk_x_c, gamma) e(C_c, delta), vk_x_c = IC_0 + sum_i x_{c,i} IC_{i+1}.  The call
 * tests, with r_c = a_c + b_c z^2 from rand[2c], rand[2c + 1] exactly as zkp_pairing_check_batch_rlc forms them (draw them uniformly at
 * random, per call, from a cryptographic source), s_0 = sum_c r_c and s_{i+1} = sum_c r_c x_{c,i} (mod r):
 *     prod_c e([r_c] A_c, B_c) * e(-sum_c [r_c] C_c, delta) * e(-sum_i [s_i] IC_i, gamma) * e(-[s_0] alpha, beta) == 1
 * *all_ok = that test AND every point valid AND every public input < r AND no (a_c, b_c) = (0, 0): 1 implies, with probability at
 * least 1 - 2^-128, that every proof is valid, and a batch of valid proofs always gives 1.  Points are in wire format; key points are
 * finite (a key has no infinity flags); the inf_* arrays of the batch may be NULL.  An invalid point, a public input >= r (x + r is
 * not x to a verifier) and a zero (a, b) are RESULTS (*all_ok = 0), not errors, in either validation mode; coordinates >= p keep the
 * rule above (ZKP_ERR_NONCANONICAL / the validation word when validation is on).  Unless flags says otherwise every proof point
 * (ZKP_GROTH16_POINTS_CHECKED) and every key point (ZKP_GROTH16_VK_CHECKED) goes through is_valid first.  n == 0 gives 1; n_inputs == 0
 * is legal (vk_x = IC_0).  ZKP_ERR_ARG: null pointers with non-zero counts, n > 2^24, n_inputs > 65535, n n_inputs > 2^31 - 1, unknown
 * flags.  Cost: n endomorphism scalings and one Miller product over the n free pairs, one G1 MSM of n terms (the C column), the fold, one
 * MSM call of two sums of n_inputs + 1 terms (the IC sum and [s_0] alpha), one Miller product over three pairs, ONE final exponentiation.
 * The signs are handled on the device (the three G2 key points are negated): there is no host-side "prepare" step.  The _dev flavour
 * is asynchronous (no read-back) and capturable into a hipGraph once the context's workspaces have reached the call's size; d_all_ok
 * (one int32) is required.  Workspace (grow-only, zkp_groth16_plan.hpp) per proof: 32 B of scalar, 97 B of scaled point, 3 B of status
 * without ZKP_GROTH16_POINTS_CHECKED; per public input 257 B; the fold's partial sums (above); plus the MSM workspace of n terms (about
 * 1.0 KB per term) and the Miller loop's own workspace. */
typedef enum {
    ZKP_FR_MUL = 0,
    ZKP_FR_ADD = 1,
    ZKP_FR_SUB = 2,
    ZKP_FR_NEG = 3,
    ZKP_FR_SQUARE = 4,
    ZKP_FR_INVERT = 5       /* 0 gives 0 (the reference returns None, src/fr.rs:266-362) */
} zkp_fr_op;
typedef struct {
    const void *alpha_g1, *beta_g2, *gamma_g2, *delta_g2;   /* one point each */
    size_t n_inputs;
    const void* ic;                                         /* n_inputs + 1 G1 points */
} zkp_groth16_vk;
typedef struct {
    size_t n;
    const void *a, *inf_a, *b, *inf_b, *c, *inf_c;          /* n G1, n G2, n G1 (+ optional infinity bytes) */
    const void* inputs;                                     /* n x n_inputs x 4 u64, one row per proof */
} zkp_groth16_batch;
#define ZKP_GROTH16_POINTS_CHECKED 1   /* flags: the proof points are known valid */
#define ZKP_GROTH16_VK_CHECKED     2   /* flags: the key points are known valid */
int zkp_fr_op_batch(zkp_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
int zkp_fr_op_batch_dev(zkp_ctx* ctx, int op, const void* d_a, const void* d_b, size_t n, void* d_out, void* stream);
int zkp_fr_from_wide_batch(zkp_ctx* ctx, const uint8_t* bytes /* 64 B little-endian each */, size_t n, uint64_t* out);
int zkp_fr_from_wide_batch_dev(zkp_ctx* ctx, const void* d_bytes, size_t n, void* d_out, void* stream);
int zkp_fr_fold_batch(zkp_ctx* ctx, const uint64_t* w /* n x 4 */, const uint64_t* x /* n x l x 4, row per w */, size_t n, size_t l,
                      uint64_t* out /* l x 4 */, uint64_t* sum_w /* 4 u64, may be NULL */);
int zkp_fr_fold_batch_dev(zkp_ctx* ctx, const void* d_w, const void* d_x, size_t n, size_t l, void* d_out, void* d_sum_w, void* stream);
/* host flavour: the key's and the batch's pointers are host arrays */
int zkp_groth16_verify_batch(zkp_ctx* ctx, const zkp_groth16_vk* vk, const zkp_groth16_batch* b, const uint64_t* rand /* 2 u64 per proof */,
                             int flags, int* all_ok);
/* device flavour: the key's and the batch's pointers, d_rand and d_all_ok are device pointers (the descriptors are host structs) */
int zkp_groth16_verify_batch_dev(zkp_ctx* ctx, const zkp_groth16_vk* vk, const zkp_groth16_batch* b, const void* d_rand, int flags,
                                 void* d_all_ok, void* stream);

/* ---- batched Fr inversion, barycentric evaluation and the batch KZG opening verifier (symbols added under ABI version 4) ----------------
 * zkp_fr_invert_batch: out[i] = a[i]^-1 mod r, and 0 for 0: bit for bit what zkp_fr_op_batch(ZKP_FR_INVERT) gives, by Montgomery's trick
 * (zkvm_pairings_amd/csrc/zkp_kzg.hip): a thread multiplies up a run of 4 consecutive elements, a workgroup its 256 run totals over LDS, one
 * middle launch the workgroup totals, where the call's ONE power r - 2 is taken; a back-sweep gives the inverses.  out may be exactly a (in
 * place); any other overlap is the caller's error.  n <= 2^31 - 1, else ZKP_ERR_ARG; n == 0 is legal.  Validation mode as zkp_fr_op_batch.
 * Cost: at most 8 Montgomery products per element (7.25 in a full workgroup of 1024) and one power per call, against about 380 products per
 * element for ZKP_FR_INVERT; no atomics; exact, so the result does not depend on the grid.  Workspace (grow-only, layout
 * zkvm_pairings_amd/csrc/zkp_kzg_plan.hpp): 64 B per 1024 elements.  The _dev flavour is asynchronous and capturable into a hipGraph once that
 * workspace has reached the call's size.
 * zkp_fr_eval_batch: n_poly polynomials, each given by its N = 2^log2_n evaluations f_{j,i} over the domain {w^i}, w = 7^((r - 1) / N), at one
 * point z_j each: out[j] = (z_j^N - 1) / N * sum_i f_{j,i} w^i / (z_j - w^i), and f_{j,i} where z_j = w^i (found on the device, from the zero
 * denominator).  With ZKP_FR_EVAL_BITREV evaluation i belongs to w^bitrev(i) (log2_n bits reversed), the order blobs are stored in.
 * log2_n <= 20, n_poly N <= 2^26, unknown flags: ZKP_ERR_ARG, refused before a byte is read; n_poly == 0 is legal.  Inputs are canonical
 * (validation mode as above).  The domain table (32 B N, built on the device the first time a call needs that many points) and the workspace
 * (32 B per evaluation for the denominators, which are inverted in place by the routine above, plus that routine's 64 B per 1024) are kept by
 * the context.  The _dev flavour is asynchronous and capturable after a first call of that size.
 * zkp_kzg_verify_batch: n openings (C_i, z_i, y_i, pi_i) - commitment, point, value, proof - against ONE setup (g1, g2, [tau]g2).  Opening i
 * holds iff e(C_i - [y_i]g1 + [z_i]pi_i, g2) == e(pi_i, [tau]g2).  The call tests, with r_i = a_i + b_i z^2 from rand[2i], rand[2i + 1] exactly
 * as zkp_pairing_check_batch_rlc forms them (draw them uniformly at random, per call, from a cryptographic source), t_i = r_i z_i mod r and
 * u = sum_i r_i y_i mod r:
 *     e(sum_i [r_i] C_i + sum_i [t_i] pi_i - [u] g1, -g2) * e(sum_i [r_i] pi_i, [tau]g2) == 1
 * *all_ok = that test AND every point valid AND every z_i, y_i < r AND no (a_i, b_i) = (0, 0): 1 implies, with probability at least
 * 1 - 2^-128, that every opening holds, and a batch of true openings always gives 1.  The setup points are finite; the inf_* arrays of the batch
 * may be NULL; a flagged infinity is a valid point (the zero polynomial opens as C = infinity, y = 0, pi = infinity).  An invalid point, a z or y
 * >= r and a zero (a, b) are RESULTS (*all_ok = 0), not errors, in either validation mode; coordinates >= p keep the library's rule
 * (ZKP_ERR_NONCANONICAL / the validation word when validation is on).  Unless flags says otherwise every C_i and pi_i
 * (ZKP_KZG_POINTS_CHECKED) and g1, g2, [tau]g2 (ZKP_KZG_VK_CHECKED) go through is_valid first.  n == 0 gives 1.  ZKP_ERR_ARG: null pointers
 * with a non-zero count, n > 2^22, unknown flags.  Cost: 2 n Fr products and the fold of u, one shared-bases G1 MSM call of two sums over 2 n + 1 points
 * (two calls at n = 2^22), one Miller product over two pairs, ONE final exponentiation; the sign is handled on the device (g2 is negated).  The _dev flavour is asynchronous
 * (no read-back) and capturable into a hipGraph once the context's workspaces have reached the call's size; d_all_ok (one int32) is required.
 * Workspace (grow-only, zkp_kzg_plan.hpp) per opening: 128 B of scalars, 194 B of copied points and flags, 2 B of status without
 * ZKP_KZG_POINTS_CHECKED; plus the MSM workspace of 2 n + 1 terms and the Miller loop's own. */
#define ZKP_FR_EVAL_BITREV 1           /* flags: evaluation i belongs to w^bitrev(i) */
typedef struct {
    const void *g1, *g2, *tau_g2;                           /* one finite point each */
} zkp_kzg_vk;
typedef struct {
    size_t n;
    const void *c, *inf_c, *proof, *inf_proof;              /* n G1, n G1 (+ optional infinity bytes) */
    const void *z, *y;                                      /* n x 4 u64 each */
} zkp_kzg_batch;
#define ZKP_KZG_POINTS_CHECKED 1       /* flags: the commitments and proofs are known valid */
#define ZKP_KZG_VK_CHECKED     2       /* flags: the setup points are known valid */
int zkp_fr_invert_batch(zkp_ctx* ctx, const uint64_t* a, size_t n, uint64_t* out);
int zkp_fr_invert_batch_dev(zkp_ctx* ctx, const void* d_a, size_t n, void* d_out, void* stream);
int zkp_fr_eval_batch(zkp_ctx* ctx, const uint64_t* evals /* n_poly x N x 4 */, const uint64_t* z /* n_poly x 4 */, size_t n_poly, unsigned log2_n,
                      int flags, uint64_t* out /* n_poly x 4 */);
int zkp_fr_eval_batch_dev(zkp_ctx* ctx, const void* d_evals, const void* d_z, size_t n_poly, unsigned log2_n, int flags, void* d_out, void* stream);
/* host flavour: the setup's and the batch's pointers are host arrays */
int zkp_kzg_verify_batch(zkp_ctx* ctx, const zkp_kzg_vk* vk, const zkp_kzg_batch* b, const uint64_t* rand /* 2 u64 per opening */, int flags,
                         int* all_ok);
/* device flavour: the setup's and the batch's pointers, d_rand and d_all_ok are device pointers (the descriptors are host structs) */
int zkp_kzg_verify_batch_dev(zkp_ctx* ctx, const zkp_kzg_vk* vk, const zkp_kzg_batch* b, const void* d_rand, int flags, void* d_all_ok,
                             void* stream);
/* the producer side - the batched Fr NTT and the KZG opening - is declared in zkp_poly.h, a second header of this library */
/* the Groth16 producer side - the Fr sparse product, the QAP quotient, the batched prover - is declared in zkp_prove.h, a third header */
/* the group-transform layer - the batched NTT over G1 points and the FK20 proofs at every domain point - is declared in zkp_fk20.h, a fourth header */
/* the cell layer - FK20 multi-proofs on cosets of the extended domain and their batch verifier - is declared in zkp_cells.h, a fifth header */
/* the recovery layer - erased blobs back from any half of their cells - is declared in zkp_recover.h, a sixth header */

/* ---- uncompressed point byte codec (big-endian field elements, reference src/fp.rs:165-207 with the range
 * check done CORRECTLY - upstream's Fp::from_bytes accepts exactly the non-canonical values).
 * G1: x(48) | y(48) = 96 bytes; G2: x.c1 | x.c0 | y.c1 | y.c0 = 192 bytes (c1 first, the usual BLS12-381
 * serialisation order).  The top three bits of byte 0 are flags: 0x80 compressed (rejected here; zkp_g*_decompress_batch below), 0x40 infinity
 * (all other bytes must be zero), 0x20 must be clear.
 * status[i]: 0 ok, 1 coordinate >= p, 2 bad flags / malformed infinity.  Decoded points go out in wire
 * format (+ infinity byte) and can be fed to zkp_g*_is_valid_batch / zkp_pairing_*. */
int zkp_g1_decode_batch(zkp_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* out_g1, uint8_t* out_inf, uint8_t* status);
int zkp_g2_decode_batch(zkp_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* out_g2, uint8_t* out_inf, uint8_t* status);
int zkp_g1_encode_batch(zkp_ctx* ctx, const uint64_t* g1, const uint8_t* inf, size_t n, uint8_t* out_bytes);
int zkp_g2_encode_batch(zkp_ctx* ctx, const uint64_t* g2, const uint8_t* inf, size_t n, uint8_t* out_bytes);

/* batched field op in the zkVM precompile shape (op: zkp_fp_op; 0 = mul and 1 = add as in src/fp.rs:376,443) */
int zkp_fp_op_batch(zkp_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* batched tower operation (op: zkp_tower_op) on the context's kernel family; a, b, out: n records of 72 u64; b is read
 * only by the binary operations; repeat only by ZKP_TOWER_FP12_CYCLOTOMIC_POW2K. */
int zkp_tower_op_batch(zkp_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint32_t repeat, uint64_t* out);

/* ---- device-pointer entry points (buffers already resident in HBM; asynchronous on `stream`) ---- */
/* `stream` is a hipStream_t passed as void* (NULL = default stream).  Same formats as above. */
/* hipGraph capture (round 6): a `_dev` call on a stream that is being captured enqueues kernel nodes and, in some paths, memset and
 * device-to-device copy nodes (the points check's counter, the RLC's fixed points and flags, the 576-byte results of the product calls;
 * tests/test_gpu_graph_replay.py replays every entry point repeatedly on changed inputs) - no allocation once
 * the context's workspaces have reached the call's size (run the call once outside the capture first), no host synchronisation, and
 * the internal pipeline streams join the capture through their fork / join events.  The hand-over of the context's workspace between
 * calls on DIFFERENT streams (an event per context) is skipped under capture: order a replayed graph against the context's other
 * calls yourself.  Measured (profiles/r06/v58_trace_n1.txt): launch gaps are 0.7 % of a single pairing's 3.8 ms - the kernels are
 * bound by one wavefront's dependent instruction chain - and a captured call replays in 3.50 ms against 3.54 ms plain (bench line,
 * batch_sweep.rows[].hipgraph): capture is supported, the library itself keeps no graph cache. */
int zkp_pairing_batch_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, const void* d_inf1, const void* d_inf2,
                          size_t n, void* d_out_gt, void* stream);
int zkp_multi_miller_loop_batch_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, const void* d_inf1,
                                    const void* d_inf2, size_t n_checks, size_t k, void* d_out_ml, void* stream);
int zkp_final_exponentiation_batch_dev(zkp_ctx* ctx, const void* d_f, size_t n, void* d_out_gt, void* stream);
/* d_ok: n_checks bytes (may be NULL); d_all_ok: one int32 written with the AND (may be NULL). */
int zkp_pairing_check_batch_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, const void* d_inf1,
                                const void* d_inf2, size_t n_checks, size_t k, void* d_ok, void* d_all_ok,
                                void* stream);
/* pairing() and the Gt::identity() check in one pass: Gt out (may be NULL) + ok bytes + AND flag. */
int zkp_pairing_gt_check_batch_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, const void* d_inf1,
                                   const void* d_inf2, size_t n_checks, size_t k, void* d_out_gt, void* d_ok,
                                   void* d_all_ok, void* stream);
/* device flavours of the one-product-check entry points; d_out_ml / d_out: 72 u64; d_out_gt (may be NULL): 72 u64;
 * d_is_one (may be NULL): one int32. */
int zkp_miller_product_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, const void* d_inf1, const void* d_inf2,
                           size_t n, void* d_out_ml, void* stream);
int zkp_fp12_product_dev(zkp_ctx* ctx, const void* d_f, size_t n, void* d_out, void* stream);
int zkp_pairing_product_check_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, const void* d_inf1,
                                  const void* d_inf2, size_t n, void* d_out_gt, void* d_is_one, void* stream);
int zkp_g1_is_valid_batch_dev(zkp_ctx* ctx, const void* d_g1, const void* d_inf, size_t n, void* d_status, void* stream);
int zkp_g2_is_valid_batch_dev(zkp_ctx* ctx, const void* d_g2, const void* d_inf, size_t n, void* d_status, void* stream);
int zkp_g1_mul_batch_dev(zkp_ctx* ctx, const void* d_base, size_t base_stride, const void* d_scalars, size_t n,
                         void* d_out, void* d_out_inf, void* stream);
int zkp_g2_mul_batch_dev(zkp_ctx* ctx, const void* d_base, size_t base_stride, const void* d_scalars, size_t n,
                         void* d_out, void* d_out_inf, void* stream);

/* addition and MSM on resident buffers (same formats and limits as zkp_g*_add_batch / zkp_g*_msm_batch above).  Capturable into a hipGraph
 * once the context's MSM workspace has reached the call's size. */
int zkp_g1_add_batch_dev(zkp_ctx* ctx, const void* d_a, const void* d_inf_a, const void* d_b, const void* d_inf_b, size_t n, void* d_out,
                         void* d_out_inf, void* stream);
int zkp_g2_add_batch_dev(zkp_ctx* ctx, const void* d_a, const void* d_inf_a, const void* d_b, const void* d_inf_b, size_t n, void* d_out,
                         void* d_out_inf, void* stream);
int zkp_g1_msm_batch_dev(zkp_ctx* ctx, const void* d_points, const void* d_inf, const void* d_scalars, size_t m, size_t n_msm, int shared_bases,
                         void* d_out, void* d_out_inf, void* stream);
int zkp_g2_msm_batch_dev(zkp_ctx* ctx, const void* d_points, const void* d_inf, const void* d_scalars, size_t m, size_t n_msm, int shared_bases,
                         void* d_out, void* d_out_inf, void* stream);
/* measurement: zkp_g*_msm_batch_dev (which = 1 / 2) that synchronises and reports the milliseconds of its six phases, summed over its passes:
 * phase_ms[0] point conversion, [1] digits, [2] sort, [3] bucket sums, [4] bucket reduction, [5] window combination + affine output */
int zkp_msm_profile_dev(zkp_ctx* ctx, int which, const void* d_points, const void* d_inf, const void* d_scalars, size_t m, size_t n_msm,
                        int shared_bases, void* d_out, void* d_out_inf, void* stream, float* phase_ms);

/* the uncompressed point codec on resident buffers (same formats and status bytes as zkp_g1/g2_decode_batch above) */
int zkp_g1_decode_batch_dev(zkp_ctx* ctx, const void* d_bytes, size_t n, void* d_out_g1, void* d_out_inf, void* d_status, void* stream);
int zkp_g2_decode_batch_dev(zkp_ctx* ctx, const void* d_bytes, size_t n, void* d_out_g2, void* d_out_inf, void* d_status, void* stream);
int zkp_g1_encode_batch_dev(zkp_ctx* ctx, const void* d_g1, const void* d_inf /* may be NULL */, size_t n, void* d_out_bytes, void* stream);
int zkp_g2_encode_batch_dev(zkp_ctx* ctx, const void* d_g2, const void* d_inf /* may be NULL */, size_t n, void* d_out_bytes, void* stream);

/* ---- BASELINE config 5 as ONE call: raw uncompressed points -> decode -> is_valid -> pairing check ------------------------------
 * n_checks groups of k consecutive (G1, G2) pairs given as byte strings (96 B per G1 point, 192 B per G2 point, the codec's format).
 * Every point is decoded (Fp::from_bytes with the correct range check, src/fp.rs:165-207) and validated (G1Affine::is_valid
 * src/g1.rs:49-62, G2Affine::is_valid src/g2.rs:57-69); st1[i] / st2[i] (n_checks * k bytes each, may be NULL) receive a
 * zkp_point_status.  ok[c] = (every point of check c is valid AND prod_j e(P_cj, Q_cj) == Gt::identity()); *all_ok = AND over the
 * checks (each may be NULL).  A point that is not valid takes no part in the Miller loop (no arithmetic on garbage); its check
 * fails.  Decoded points, infinity flags and intermediate status bytes stay in the context's workspace in HBM: the host flavour
 * moves only the byte strings up and the status / ok bytes down.
 * Validate first, then use (ABI version 4): only the checks whose 2k points are all valid enter the Miller loop and the final
 * exponentiation - they are listed and gathered on the device, so a check with an invalid point costs its validity tests and nothing
 * more.  The NUMBER of listed checks never leaves the device (round 6): the pairing phase is launched for the worst case and its
 * kernels read the count themselves, so the `_dev` flavour is asynchronous on `stream` like every other `_dev` call (no host
 * read-back, capturable into a hipGraph once the context's workspaces have reached their size: the first call of a size allocates). */
typedef enum {
    ZKP_POINT_OK = 0,               /* a point of the r-torsion subgroup, or a well-formed infinity */
    ZKP_POINT_NONCANONICAL = 1,     /* a coordinate >= p */
    ZKP_POINT_MALFORMED = 2,        /* compressed / sort flag set, or an infinity flag over non-zero bytes */
    ZKP_POINT_NOT_ON_CURVE = 3,     /* "Point is not on curve", src/g1.rs:54-56 */
    ZKP_POINT_NOT_IN_SUBGROUP = 4   /* "Point is not torsion free", src/g1.rs:57-59 */
} zkp_point_status;
int zkp_points_check_batch(zkp_ctx* ctx, const uint8_t* g1_bytes, const uint8_t* g2_bytes, size_t n_checks, size_t k, uint8_t* st1,
                           uint8_t* st2, uint8_t* ok, int* all_ok);
int zkp_points_check_batch_dev(zkp_ctx* ctx, const void* d_g1_bytes, const void* d_g2_bytes, size_t n_checks, size_t k, void* d_st1,
                               void* d_st2, void* d_ok, void* d_all_ok, void* stream);

/* ---- compressed points (48 B per G1 point, 96 B per G2 point): square roots, codec, points check -------------------------------
 * The usual BLS12-381 compressed serialisation: x only, big-endian, G2 as x.c1 | x.c0 (c1 first, as the uncompressed codec).  The top
 * three bits of byte 0 are flags: 0x80 compressed (must be set, else status 2), 0x40 infinity (every other bit of the string, the sort
 * flag included, must be zero, else status 2), 0x20 sort flag = y is the lexicographically larger of y and -y (G1: y > (p-1)/2; G2:
 * compare c1, and c0 when c1 == 0).
 * Decompression: status[i] (zkp_point_status) 0 ok, 1 x (either coordinate on G2) >= p, 2 bad flags / malformed infinity,
 * 3 x^3 + b has no square root (ZKP_POINT_NOT_ON_CURVE).  Otherwise the root the sort flag selects: the unique point (x, y) on the
 * curve; y = 0 (possible on G2 only) decodes to (x, 0) whatever the flag says.  The subgroup is NOT checked (is_valid does that, as
 * after zkp_g*_decode_batch).  Output: the wire formats above + infinity byte; the identity decodes to (0, 1); rejected points to 0.
 * Compression reads x and the sign of y only: it does not assume the point is valid.  inf may be NULL.
 * The square roots stand in for Fp::sqrt (src/fp.rs:280-300: a^((p+1)/4), checked by squaring) and Fp2::sqrt (src/fp2.rs:231-273,
 * step for step, the alpha == -1 branch included): out[i] is the reference's root bit for bit, or zero where the reference returns
 * Err / None; is_square[i] = 1 iff it returns Ok / Some.  Host pointers only, like zkp_fp_op_batch; validation mode applies.
 * zkp_points_check_compressed_batch[_dev] is zkp_points_check_batch[_dev] with decompression as its decode step: same status bytes,
 * same validate-first compaction, same device-resident count (the _dev flavour is asynchronous and capturable). */
int zkp_fp_sqrt_batch(zkp_ctx* ctx, const uint64_t* a, size_t n, uint64_t* out, uint8_t* is_square);    /* src/fp.rs:280-300 */
int zkp_fp2_sqrt_batch(zkp_ctx* ctx, const uint64_t* a, size_t n, uint64_t* out, uint8_t* is_square);   /* src/fp2.rs:231-273 */
int zkp_g1_decompress_batch(zkp_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* out_g1, uint8_t* out_inf, uint8_t* status);
int zkp_g2_decompress_batch(zkp_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* out_g2, uint8_t* out_inf, uint8_t* status);
int zkp_g1_compress_batch(zkp_ctx* ctx, const uint64_t* g1, const uint8_t* inf, size_t n, uint8_t* out_bytes);
int zkp_g2_compress_batch(zkp_ctx* ctx, const uint64_t* g2, const uint8_t* inf, size_t n, uint8_t* out_bytes);
int zkp_g1_decompress_batch_dev(zkp_ctx* ctx, const void* d_bytes, size_t n, void* d_out_g1, void* d_out_inf, void* d_status, void* stream);
int zkp_g2_decompress_batch_dev(zkp_ctx* ctx, const void* d_bytes, size_t n, void* d_out_g2, void* d_out_inf, void* d_status, void* stream);
int zkp_g1_compress_batch_dev(zkp_ctx* ctx, const void* d_g1, const void* d_inf /* may be NULL */, size_t n, void* d_out_bytes, void* stream);
int zkp_g2_compress_batch_dev(zkp_ctx* ctx, const void* d_g2, const void* d_inf /* may be NULL */, size_t n, void* d_out_bytes, void* stream);
int zkp_points_check_compressed_batch(zkp_ctx* ctx, const uint8_t* g1_bytes, const uint8_t* g2_bytes, size_t n_checks, size_t k, uint8_t* st1,
                                      uint8_t* st2, uint8_t* ok, int* all_ok);
int zkp_points_check_compressed_batch_dev(zkp_ctx* ctx, const void* d_g1_bytes, const void* d_g2_bytes, size_t n_checks, size_t k, void* d_st1,
                                          void* d_st2, void* d_ok, void* d_all_ok, void* stream);

/* validation mode (zkp_set_validate) on the device-pointer entry points: the range check of the inputs runs on the caller's
 * stream and ORs into a word inside the context - no host synchronisation in the *_dev call itself.  This call waits for
 * `stream`, reports whether any *_dev call since the last query saw a field element >= p (*bad = 1; the results of such a
 * call are unspecified) and clears the word. */
int zkp_take_validation_status_dev(zkp_ctx* ctx, void* stream, int* bad);

/* ---- several GPUs behind one call ------------------------------------------------------------------
 * ONE host thread, n_ctx distinct contexts (normally one per GPU of the node, each from zkp_init(device)); the checks
 * are split into contiguous blocks, one per context (a check's k pairs and its shared final exponentiation stay
 * on one GPU), every context uploads, computes and downloads its block on its own stream concurrently, and the
 * per-context AND flags are combined on the host - the data path has no collective.  Host pointers, synchronous,
 * same formats and results as zkp_pairing_check_batch / zkp_pairing_batch + the Gt::identity() flags.
 * The one-process-per-GPU form (torchrun / MPI ranks) is zkp_pairing_check_batch per rank followed by ONE
 * ncclAllReduce(&flag, &flag, 1, ncclInt32, ncclMin, comm, stream): RCCL has no bitwise AND, MIN of {0,1} is AND. */
int zkp_pairing_check_batch_multi(zkp_ctx* const* ctxs, int n_ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1,
                                  const uint8_t* inf2, size_t n_checks, size_t k, uint8_t* ok /* may be NULL */, int* all_ok);
/* out_gt[i] = pairing(g1[i], g2[i]); ok[i] = (out_gt[i] == Gt::identity()) and *all_ok, each optional */
int zkp_pairing_batch_multi(zkp_ctx* const* ctxs, int n_ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1,
                            const uint8_t* inf2, size_t n, uint64_t* out_gt, uint8_t* ok, int* all_ok);

/* ---- one process (rank) per GPU: the path's ONE collective behind the C ABI ------------------------------------
 * librccl is linked into libzkp_pairings.so; a Rust / C host needs nothing outside this header to finish a sharded check:
 *     rank 0: zkp_comm_unique_id(id)            -> hand the 128 bytes to every rank by the host's own means (file, socket, MPI)
 *     every rank: zkp_comm_init_rank(ctx, nranks, rank, id)        (collective: returns when all ranks have joined)
 *     every rank: zkp_pairing_check_batch_allreduce(ctx, <its contiguous block of the checks>, ok, &all_ok)
 * = zkp_pairing_check_batch on the rank's block, then ONE ncclAllReduce(count = 1, ncclInt32, ncclMin) of the AND flag on the
 * context's stream (RCCL has no bitwise AND; MIN of {0,1} is AND): *all_ok is the AND over ALL ranks' checks, ok[] stays
 * per-rank.  Nothing else crosses xGMI.  A context holds at most one communicator; zkp_free destroys it.
 * Failure on one rank: a rank whose OWN block fails (bad arguments, non-canonical limbs under zkp_set_validate, a HIP error) still
 * takes part in the collective - with flag 0 (AND-reduce) or the zero record (all-gather variant) - so no peer is left waiting and
 * every rank reads all_ok / is_one = 0; the failing rank returns its own status afterwards.  Only a call without context,
 * output flag or communicator returns before the collective (ZKP_ERR_ARG / ZKP_ERR_COMM).
 * zkp_comm_init_rank itself is a collective: every rank must call it (a rank that cannot - no context, no device - makes the others
 * wait, as with any bootstrap).  Its local failures come AFTER the bootstrap (round 6): a rank without memory for the communicator's
 * records aborts its side and returns ZKP_ERR_OOM; the peers cannot see that, so agree on the ranks' statuses over the host's own
 * channel before the first collective (bench.py does: one gloo all-reduce(MIN) of "init ok").  No reference
 * counterpart (the reference is a single-threaded host crate); the torch.distributed flavour of the same step is
 * zkvm_pairings_amd/dist.py. */
#define ZKP_COMM_ID_BYTES 128
int zkp_comm_unique_id(void* out_id /* ZKP_COMM_ID_BYTES */);
int zkp_comm_init_rank(zkp_ctx* ctx, int nranks, int rank, const void* unique_id /* ZKP_COMM_ID_BYTES */);
int zkp_comm_destroy(zkp_ctx* ctx);
/* *nranks = 0 when the context has no communicator */
int zkp_comm_info(const zkp_ctx* ctx, int* nranks, int* rank);
/* in-place AND of one int32 {0,1} flag in device memory over the ranks, asynchronous on `stream` (the building block) */
int zkp_and_allreduce_dev(zkp_ctx* ctx, void* d_flag, void* stream);
int zkp_pairing_check_batch_allreduce(zkp_ctx* ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2,
                                      size_t n_checks, size_t k, uint8_t* ok /* may be NULL */, int* all_ok);
/* d_all_ok (one int32, required) receives the AND over all ranks; asynchronous on `stream` */
int zkp_pairing_check_batch_allreduce_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, const void* d_inf1, const void* d_inf2,
                                          size_t n_checks, size_t k, void* d_ok, void* d_all_ok, void* stream);
/* pairing() + the Gt::identity() check of this rank's block (zkp_pairing_gt_check_batch_dev: Gt out, may be NULL, + ok bytes) and the
 * same ONE all-reduce of the AND flag - BASELINE config 3 ("2^20 pairings sharded across 8 GPUs with RCCL AND-reduce of Gt==identity")
 * as one call per rank; it is the step `bench.py --collective abi` times.  d_all_ok is required.  (ABI version 4) */
int zkp_pairing_gt_check_batch_allreduce_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, const void* d_inf1, const void* d_inf2,
                                             size_t n_checks, size_t k, void* d_out_gt, void* d_ok, void* d_all_ok, void* stream);
/* BASELINE config 5 on a node ("subgroup check + pairing on raw points, 8 GPUs"): this rank's block of zkp_points_check_batch, then the
 * same ONE all-reduce of the AND flag; status and ok bytes stay per rank.  d_all_ok / all_ok are required. */
int zkp_points_check_batch_allreduce(zkp_ctx* ctx, const uint8_t* g1_bytes, const uint8_t* g2_bytes, size_t n_checks, size_t k, uint8_t* st1,
                                     uint8_t* st2, uint8_t* ok, int* all_ok);
int zkp_points_check_batch_allreduce_dev(zkp_ctx* ctx, const void* d_g1_bytes, const void* d_g2_bytes, size_t n_checks, size_t k,
                                         void* d_st1, void* d_st2, void* d_ok, void* d_all_ok, void* stream);
/* SURVEY.md 8e variant, ONE product check over the whole sharded batch: this rank's zkp_miller_product, ONE ncclAllGather of
 * 576 B per rank, the product of the gathered values and ONE final exponentiation on every rank (identical results):
 * *is_one = (prod over ALL ranks' pairs of e(P_i, Q_i) == Gt::identity()); out_gt (72 u64) may be NULL. */
int zkp_pairing_product_check_allgather(zkp_ctx* ctx, const uint64_t* g1, const uint64_t* g2, const uint8_t* inf1, const uint8_t* inf2,
                                        size_t n, uint64_t* out_gt, int* is_one);

/* ---- pinned host memory for the host-pointer entry points ("H2D/D2H per GPU straight from pinned host
 * memory on its own stream") ------------------------------------------------------------------------------------------
 * The host-pointer entry points copy with hipMemcpyAsync on their own streams.  From PAGEABLE memory such a copy stages
 * through a driver buffer and blocks the calling thread, so the next slice's upload (zkp_pairing_batch) or the next
 * context's upload (zkp_pairing_*_multi) cannot start before it is over; from page-locked memory it is a DMA that
 * overlaps the kernels and the other contexts' copies.  zkp_host_alloc returns page-locked memory usable with every
 * context / GPU of the process (hipHostMallocPortable); zkp_host_register page-locks an existing allocation in place
 * (hipHostRegister: slow, of the order of 1 ms per 4 MB - do it once for a buffer that is reused, not per call).  The
 * registered range must consist of WHOLE PAGES of its own: ptr and bytes multiples of the page size (sysconf(_SC_PAGESIZE),
 * 4096 on the GPU boxes; zkp_host_unregister(NULL) is ZKP_ERR_ARG), i.e. memory
 * from posix_memalign / aligned_alloc / mmap, not a slice of the malloc heap - the driver locks and maps pages, and two
 * registrations that share a page (two neighbouring heap arrays) left the HIP runtime with a stale entry after the
 * unregistration: a later copy from a reused heap address then went to the GPU as a DMA from an unmapped page (a GPU
 * memory fault; found in round 3).  Anything else is ZKP_ERR_ARG.  The
 * entry points themselves accept either kind of memory and give the same results.  No reference counterpart: the
 * reference is a host-only crate (its point arrays would live in a Vec; the Rust wrapper's PinnedVec in
 * integration/rust/src/lib.rs is the drop-in container). */
int zkp_host_alloc(size_t bytes, void** out_ptr);
int zkp_host_free(void* ptr);
int zkp_host_register(void* ptr, size_t bytes);
int zkp_host_unregister(void* ptr);

/* ---- measurement helper used by bench.py: times `reps` launches of the fused pairing kernel on
 * ctx's own stream with HIP events recorded on THAT stream; returns average ms per launch. ---- */
int zkp_time_pairing_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, size_t n, void* d_out_gt, int reps,
                         float* avg_ms);

/* measurement helper used by bench.py: a one-wavefront clock probe queued on `stream`; d_out (device, two u64) receives
 * the shader-clock ticks and the wall-clock ticks of about spin_us microseconds, *wall_khz the wall clock's rate.
 * Queued on a second stream beside a running pass it reports the clock the chip sustains under that load. */
int zkp_clock_probe_dev(zkp_ctx* ctx, void* stream, unsigned spin_us, void* d_out, int* wall_khz);

/* measurement: ONE pass of the fused pairing over n resident pairs with every kernel launch bracketed by HIP events on its stream
 * (a single pipeline, so that no two kernels overlap): ms[c] = summed duration and launches[c] = number of the launches of class c.
 * Cooperative family only.  bench.py prints each class against the multiply-adds it executes (roofline.kernels). */
#define ZKP_PROFILE_CLASSES 9
/* 0 k_prep_lines, 1 k_coop<30,4> (Miller program), 2 k_coop<24,34> fexp_a, 3 k_batch_inv, 4 k_ksq, 5 k_kdec_a, 6 k_kdec_b,
 * 7 k_coop<36,24> (hard-part step programs), 8 k_coop<24,34> (the other step programs of phase C) */
int zkp_profile_pairing_dev(zkp_ctx* ctx, const void* d_g1, const void* d_g2, size_t n, void* d_out_gt,
                            float* ms /* ZKP_PROFILE_CLASSES */, int* launches /* ZKP_PROFILE_CLASSES */);

/* diagnostic: time one synthetic step program of the cooperative interpreter (which: 0 T=1, 1 T=3,
 * 2 T=3+epilogue, 3 T=6, 4 T=12, 5 LIN, 6 / 7 cyclotomic squaring without / with companion slots, 8 spill + fill;
 * 9: 400 compressed squarings of k_ksq; 10: the line precomputation k_prep_lines of n pairs; 11: the one-pair Miller
 * program over the line stream that 10 left behind - n at most one chunk, 65536 by default; 15: like 10 with the upstream-shaped
 * lines of multi_miller_loop(), k_prep_lines<false>) over n checks, on ctx's own
 * stream with its own events; used by tools/ and by bench.py's per-kernel roofline split. */
int zkp_time_coop_step(zkp_ctx* ctx, int which, size_t n, float* ms);

#ifdef __cplusplus
}
#endif
#endif
