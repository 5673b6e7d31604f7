/*
 * include/zkp_poly.h -- the polynomial / producer layer of libzkp_pairings.so: the batched NTT over the BLS12-381 scalar field and
 * the producer side of KZG (commit and open).  A second header of the SAME library: include it beside zkp_pairings.h, whose
 * zkp_ctx, zkp_status codes, zkp_set_validate, validation word (zkp_take_validation_status_dev) and wire formats apply unchanged.
 * Symbols added under ABI version 4 (zkp_abi_version() is still 4).
 *
 * Each entry point has a host-pointer flavour and a _dev flavour with a trailing stream.  The _dev flavour is asynchronous, reads
 * nothing back, and is capturable into a hipGraph once the context's workspaces have reached the call's size (run the call once
 * before capturing it) - the contract of zkp_fr_eval_batch_dev.  Elements are uint64_t[4], little-endian, canonical (< r); in
 * validation mode an element >= r gives ZKP_ERR_NONCANONICAL on the host flavour and ORs into the validation word on the _dev one.
 *
 * zkp_fr_ntt_batch: n_poly polynomials of N = 2^log2_n coefficients each.  Forward: out[j][i] = sum_k in[j][k] (s w^i)^k mod r with
 * w = 7^((r - 1) / N) - the w of zkp_fr_eval_batch - and s = 1, or s = 7 with ZKP_NTT_COSET.  With ZKP_NTT_BITREV the evaluation side
 * is stored bit-reversed: slot i belongs to s w^bitrev(i), the order of ZKP_FR_EVAL_BITREV.  ZKP_NTT_INVERSE is the exact inverse map
 * under the same other flags (evaluations in, coefficients out).  out may be exactly in; any other overlap is the caller's error.
 * ZKP_ERR_ARG, before a byte is read: log2_n > 20, n_poly N > 2^26, unknown flags, null pointers with a non-zero count.  n_poly == 0
 * is legal, log2_n == 0 is the identity.
 * How (zkvm_pairings_amd/csrc/zkp_poly.hip, zkp_poly_plan.hpp): a workgroup takes a tile of 2^10 elements into LDS and runs all the
 * tile's stages there, four elements per thread in registers between exchanges.  Passes over the data: with ZKP_NTT_BITREV one up
 * to 2^10, two up to 2^18, three beyond, all in place; without it one up to 2^10, two up to 2^16, three beyond.  The order the flags
 * ask for comes from the decimation (in frequency, or in time for the BITREV inverse) and from the last pass's store indices, never
 * from a permutation pass.  Cost: N/2 log2 N Montgomery products per polynomial less the N/2 of the stage whose twiddles are one;
 * the coset adds at most two per element, the inverse one.  Exact; no atomics.
 * Kept by the context (grow-only): the domain table of zkp_fr_eval_batch (32 B N); the coset tables (128 KiB, built at the first
 * coset call); and, only WITHOUT ZKP_NTT_BITREV and for log2_n > 10, a workspace of 32 B n_poly N, shared with the evaluation's.
 *
 * zkp_kzg_open_batch: n polynomials in evaluation form over the N-point domain (the evaluations of zkp_fr_eval_batch, natural order or
 * ZKP_FR_EVAL_BITREV) opened at one point z_j each: out_y[j] = f_j(z_j) and out_proof[j] = [q_j(tau)] g1 for
 * q_j(X) = (f_j(X) - y_j) / (X - z_j), against the Lagrange setup lagrange_g1[i] = [l_i(tau)] g1 of the domain point evaluation slot i
 * belongs to (so a bit-reversed blob setup goes with ZKP_FR_EVAL_BITREV).  Outside the domain q_i = (f_i - y) / (w^i - z); for
 * z = w^m - found on the device from the zero the batched inversion leaves - y = f_m and
 * q_m = z^-1 sum_{i != m} (f_i - y) w^i / (z - w^i).  An infinite proof (the zero and the constant polynomials give it) is (0, 1)
 * with out_inf = 1, like every group output.  The proofs are what zkp_kzg_verify_batch consumes.
 * The setup points are TRUSTED: finite, on the curve, in the subgroup.  A producer checks its setup once with zkp_g1_is_valid_batch.
 * z and the evaluations are canonical inputs (validation mode as above).  ZKP_ERR_ARG: log2_n > 20, n N > 2^24 (the MSM's term
 * limit), unknown flags, null pointers with a non-zero count; n == 0 is legal.
 * How: the denominators, their batched inversion and the barycentric sum of zkp_fr_eval_batch; one kernel that turns the inverted
 * denominators in place into the quotient's evaluations; one shared-bases G1 MSM of the n rows over the N setup points.  A batch of
 * more than 2^22 evaluations runs in slices of whole polynomials, floor(2^22 / N) each (at least one), so the workspace is bounded:
 * 32 B per evaluation of a slice plus 64 B per 1024 (the evaluation's, at most 129 MiB) and the MSM workspace of one slice.
 *
 * Commitment needs no symbol of its own: C_j = sum_i f_{j,i} lagrange_g1[i] is zkp_g1_msm_batch with shared_bases = 1, m = N,
 * n_msm = n, the setup as points and the evaluations as scalars, in either order as long as both use the same.
 */
#ifndef ZKP_POLY_H
#define ZKP_POLY_H

#include "zkp_pairings.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKP_NTT_INVERSE 1              /* flags: evaluations in, coefficients out */
#define ZKP_NTT_BITREV  2              /* flags: the evaluation side is stored bit-reversed: slot i belongs to w^bitrev(i), as ZKP_FR_EVAL_BITREV */
#define ZKP_NTT_COSET   4              /* flags: the domain is 7 w^i (7 = the scalar field's generator) */

int zkp_fr_ntt_batch(zkp_ctx* ctx, const uint64_t* in /* n_poly x N x 4 */, size_t n_poly, unsigned log2_n, int flags, uint64_t* out /* n_poly x N x 4 */);
int zkp_fr_ntt_batch_dev(zkp_ctx* ctx, const void* d_in, size_t n_poly, unsigned log2_n, int flags, void* d_out, void* stream);

int zkp_kzg_open_batch(zkp_ctx* ctx, const uint64_t* lagrange_g1 /* N finite G1 points */, const uint64_t* evals /* n x N x 4 */,
                       const uint64_t* z /* n x 4 */, size_t n, unsigned log2_n, int flags /* ZKP_FR_EVAL_BITREV or 0 */,
                       uint64_t* out_y /* n x 4 */, uint64_t* out_proof /* n G1 */, uint8_t* out_inf /* n */);
int zkp_kzg_open_batch_dev(zkp_ctx* ctx, const void* d_lagrange_g1, const void* d_evals, const void* d_z, size_t n, unsigned log2_n, int flags,
                           void* d_out_y, void* d_out_proof, void* d_out_inf, void* stream);

#ifdef __cplusplus
}
#endif
#endif
