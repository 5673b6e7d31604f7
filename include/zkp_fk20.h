/*
 * include/zkp_fk20.h -- the group-transform layer of libzkp_pairings.so: the batched number-theoretic transform over G1 points and the
 * Feist-Khovratovich ("FK20") KZG proofs of a polynomial at EVERY point of its domain.  A fourth header of the SAME library: include it
 * beside zkp_pairings.h, whose zkp_ctx, zkp_status codes, zkp_set_validate, validation word (zkp_take_validation_status_dev) and wire
 * formats apply unchanged, and beside zkp_poly.h, whose ZKP_NTT_* flags and root of unity it shares.  Symbols added under ABI version 4
 * (zkp_abi_version() is still 4).
 *
 * Each entry point has a host-pointer flavour and a _dev flavour with a trailing stream.  The _dev flavour is asynchronous, reads
 * nothing back, and is capturable into a hipGraph once the context's workspaces and tables have reached the call's size (run the call
 * once before capturing it) - the contract of zkp_fr_eval_batch_dev.  G1 points are 12 words (x, y), the identity is (0, 1) with its flag
 * set, like every group output.  Input points are TRUSTED: on the curve and in the subgroup, the contract of the MSM; a producer checks
 * its setup once with zkp_g1_is_valid_batch.  In validation mode a coordinate >= p or a field element >= r gives ZKP_ERR_NONCANONICAL on
 * the host flavour and ORs into the validation word on the _dev one.
 *
 * zkp_g1_ntt_batch: n_vec vectors of N = 2^log2_n points each; inf (one byte per point) may be NULL: every point finite.  Forward:
 * out[j][i] = sum_k [w^(i k)] in[j][k] with w the root of zkp_fr_ntt_batch.  ZKP_NTT_INVERSE and ZKP_NTT_BITREV mean exactly what they
 * mean there (the evaluation side is stored bit-reversed; the inverse is the exact inverse map under the same other flag); there is no
 * coset.  out may be exactly points (and out_inf exactly inf); any other overlap is the caller's error.  ZKP_ERR_ARG, before a byte is
 * read: log2_n > 20, n_vec N > 2^22, unknown flags (ZKP_NTT_COSET included), null points / out / out_inf with a non-zero count.
 * n_vec == 0 is legal, log2_n == 0 is the identity map.  The inverse of the monomial setup [tau^k] g1 is the Lagrange setup
 * [l_i(tau)] g1 that the commitment and the single-point opening of zkp_poly.h consume.
 * How (zkvm_pairings_amd/csrc/zkp_fk20.hip, zkp_coop.hip, zkp_fk20_plan.hpp): one lane per butterfly on the 28-bit core, Jacobian
 * records in a workspace between the stages, every stage in place, decimation in time; the order the flags ask for comes from where the
 * first stage loads and where the last kernel stores, never from a permutation pass.  The stage whose twiddles are one multiplies
 * nothing.  Every other butterfly computes T = [w^t] B through the endomorphism - w^t = a + b z^2 mod r with a, b < 2^128 from a table of
 * the context, 128 joint doublings over B, phi'(B), B + phi'(B) - and then A + T and A - T by the full addition (A = T, A = -T and
 * infinite operands all occur on ordinary inputs).  Cost: log2 N + 1 launches; (N / 2)(log2 N - 1) 128-bit scalar multiplications and
 * N log2 N additions per vector, one field inversion per output; the inverse's [N^-1] is one more 128-bit scalar multiplication of every
 * output.  Exact; no atomics.
 * Slices and workspace: a call with a large total runs in slices of whole vectors, floor(2^18 / N) each (at least one), so the
 * workspace is bounded: 192 B per point of a slice - at most 48 MiB up to N = 2^18, 192 MiB at N = 2^20.  Kept by the context (grow-only)
 * beside it: the domain table of zkp_fr_eval_batch and the split twiddles, 32 B per domain point each, built on the device once per
 * domain size and never read back.
 *
 * zkp_kzg_fk20_setup: from the monomial setup monomial_g1[k] = [tau^k] g1, k < N = 2^log2_n, the 2 N points the proofs need: the forward
 * G1 NTT of size 2 N (natural order) of (s_{N-2}, s_{N-3}, .., s_0, then N + 1 identities).  Computed once per setup.  ZKP_ERR_ARG:
 * log2_n > 19, null pointers.  For N = 1 both outputs are the identity.
 *
 * zkp_kzg_fk20_batch: n polynomials in COEFFICIENT form (n x N x 4 words, canonical) against the output of zkp_kzg_fk20_setup
 * (fk20_setup_inf may be NULL: every point finite).  out_proof[j][m] = [q(tau)] g1 for q = (f_j - f_j(w^m)) / (X - w^m); with
 * ZKP_NTT_BITREV slot m belongs to w^bitrev(m).  The values f_j(w^m) are not an output: they are zkp_fr_ntt_batch of the same
 * coefficients.  Each proof is what zkp_kzg_verify_batch consumes, and equals the proof of the single-point opening at that point.
 * ZKP_ERR_ARG: log2_n > 19, n N > 2^21, flags other than ZKP_NTT_BITREV, null pointers with a non-zero count; n == 0 is legal.
 * How, per polynomial: c = (f_{N-1}, 0 x (N + 1), f_1, .., f_{N-2}) / (2 N); its Fr transform of size 2 N; slot by slot the 2 N scalar
 * multiplications of the setup (the 255-bit chain of zkp_g1_mul_batch, left Jacobian); the inverse G1 transform of size 2 N, unscaled -
 * the 1 / (2 N) was paid on the Fr side with one Montgomery product per element; its first N entries are h (entry N - 1 is the identity by
 * construction); the forward G1 transform of size N of h is the N proofs.  Cost: 2 N 255-bit and about (3 N / 2) log2 N 128-bit scalar
 * multiplications instead of the N multi-scalar multiplications of N terms of N single-point openings.
 * Slices and workspace: slices of whole polynomials, floor(2^17 / N) each (at least one); 224 B per point of the 2 N-point transforms of a
 * slice - at most 56 MiB up to N = 2^17, 224 MiB at N = 2^19 - and the tables above for the domain of 2 N points.
 */
#ifndef ZKP_FK20_H
#define ZKP_FK20_H

#include "zkp_poly.h"

#ifdef __cplusplus
extern "C" {
#endif

int zkp_g1_ntt_batch(zkp_ctx* ctx, const uint64_t* points /* n_vec x N G1 */, const uint8_t* inf /* n_vec x N, may be NULL */, size_t n_vec, unsigned log2_n,
                     int flags, uint64_t* out /* n_vec x N G1 */, uint8_t* out_inf /* n_vec x N */);
int zkp_g1_ntt_batch_dev(zkp_ctx* ctx, const void* d_points, const void* d_inf, size_t n_vec, unsigned log2_n, int flags, void* d_out, void* d_out_inf,
                         void* stream);

int zkp_kzg_fk20_setup(zkp_ctx* ctx, const uint64_t* monomial_g1 /* N finite G1 points */, unsigned log2_n, uint64_t* out /* 2N G1 */, uint8_t* out_inf /* 2N */);
int zkp_kzg_fk20_setup_dev(zkp_ctx* ctx, const void* d_monomial_g1, unsigned log2_n, void* d_out, void* d_out_inf, void* stream);

int zkp_kzg_fk20_batch(zkp_ctx* ctx, const uint64_t* fk20_setup /* 2N G1 */, const uint8_t* fk20_setup_inf /* 2N, may be NULL */,
                       const uint64_t* coeffs /* n x N x 4 */, size_t n, unsigned log2_n, int flags /* ZKP_NTT_BITREV or 0 */,
                       uint64_t* out_proof /* n x N G1 */, uint8_t* out_inf /* n x N */);
int zkp_kzg_fk20_batch_dev(zkp_ctx* ctx, const void* d_fk20_setup, const void* d_fk20_setup_inf, const void* d_coeffs, size_t n, unsigned log2_n, int flags,
                           void* d_out_proof, void* d_out_inf, void* stream);

#ifdef __cplusplus
}
#endif
#endif
