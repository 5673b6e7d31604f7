/*
 * include/zkp_prove.h -- the Groth16 producer side of libzkp_pairings.so: a sparse matrix times dense vectors product over the
 * BLS12-381 scalar field, the QAP quotient, and n proofs of one circuit in one call.  A third header of the SAME library: include it
 * beside zkp_pairings.h and zkp_poly.h, whose zkp_ctx, zkp_status codes, zkp_set_validate, validation word
 * (zkp_take_validation_status_dev) and wire formats apply unchanged.  Symbols added under ABI version 4 (zkp_abi_version() is still 4).
 *
 * Each entry point has a host-pointer flavour and a _dev flavour with a trailing stream.  The descriptors (zkp_fr_csr, zkp_r1cs,
 * zkp_groth16_pk) are HOST structs; the pointers inside them are host pointers in the host flavour and device pointers in the _dev
 * one.  The _dev flavour is asynchronous, reads nothing back, grows the context's workspaces first and then only launches, and is
 * capturable into a hipGraph once the workspaces have reached the call's size (run the call once before capturing it) - the contract
 * of zkp_kzg_open_batch_dev.  Elements are uint64_t[4], little-endian, canonical (< r); in validation mode an element >= r among the
 * matrix values, the witness or rs gives ZKP_ERR_NONCANONICAL on the host flavour and ORs into the validation word on the _dev one.
 *
 * Definitions.
 *   Domain    N = 2^log2_n >= n_rows, w = 7^((r - 1) / N): the w of zkp_fr_eval_batch and zkp_fr_ntt_batch.
 *   Matrices  A, B, C: n_rows x m, compressed sparse rows (row_ptr of n_rows + 1 u32, col and val of nnz entries; a column may repeat
 *             inside a row, its values add up).
 *   QAP       u_i(X) = sum_{k < n_rows} A[k][i] l_k(X) with l_k the Lagrange basis of the domain, v_i from B and w_i from C likewise;
 *             rows k >= n_rows are zero.  t(X) = X^N - 1.  NO input-consistency rows are added: this differs from arkworks and
 *             libsnark, which append one row per public variable; a caller who wants them puts them into the matrices.
 *   Witness   z in Fr^m, z_0 = 1, z_1 .. z_l public (l = n_inputs), the rest private.  a(X) = sum_i z_i u_i(X), b and c likewise.
 *             z_0 != 1 is the caller's error and is not checked.
 *   Quotient  h: the polynomial of degree < N with h(7 w^i) = (a b - c)(7 w^i) / (7^N - 1).  For a satisfying witness this is
 *             (a b - c) / t, of degree <= N - 2.  sat_j = 1 iff a(w^k) b(w^k) == c(w^k) for every k < N.
 *   Key       wire-format points: alpha_g1, beta_g1, delta_g1 (G1), beta_g2, delta_g2 (G2), a_query[m] = [u_i(tau)] g1,
 *             b_g1_query[m] = [v_i(tau)] g1, b_g2_query[m] = [v_i(tau)] g2, l_query[m - l - 1] = [(beta u_i + alpha v_i + w_i)(tau) / delta] g1
 *             for i > l, h_query[N - 1] = [tau^i t(tau) / delta] g1.  a_inf, b_g1_inf, b_g2_inf, l_inf: optional infinity bytes of the
 *             four per-variable queries (a variable absent from A or B gives an infinite entry in real keys); NULL means all finite.
 *             Key points are TRUSTED, as the KZG setup is: finite unless flagged, on the curve, in the subgroup.  Check a key once
 *             with zkp_g1_is_valid_batch / zkp_g2_is_valid_batch.
 *   Proof     with caller-supplied r_j, s_j (rs[j] = r_j | s_j, canonical): DRAW THEM UNIFORMLY AND FRESH PER PROOF for zero knowledge;
 *             0, 0 is legal and deterministic.
 *               A  = alpha_g1 + sum_i z_i a_query_i + [r] delta_g1
 *               B  = beta_g2 + sum_i z_i b_g2_query_i + [s] delta_g2
 *               B1 = beta_g1 + sum_i z_i b_g1_query_i + [s] delta_g1                      (internal, not an output)
 *               C  = sum_{i > l} z_i l_query_i + sum_{i < N - 1} h_i h_query_i + [s] A + [r] B1 - [r s] delta_g1
 *             which zkp_groth16_verify_batch accepts under the key with IC_i = [(beta u_i + alpha v_i + w_i)(tau) / gamma] g1.
 *
 * zkp_fr_spmv_batch: out[j][k] = sum_e val[e] x[j][col[e]] over the entries e of row k, for n vectors x[j] of n_cols elements; the
 * slots n_rows .. out_stride - 1 of every output row are written as zero.  ZKP_ERR_ARG, before a byte is read: n_cols > 2^22,
 * nnz > 2^31 - 1, out_stride < n_rows, out_stride > 2^20, n > 2^31 - 1, n out_stride > 2^26, null pointers with non-zero counts.
 * n == 0 and n_rows == 0 are legal.  The host flavour also checks the matrix (row_ptr[0] == 0, row_ptr monotone,
 * row_ptr[n_rows] == nnz, every col < n_cols) and returns ZKP_ERR_ARG when it is malformed.  The _dev flavour cannot (it reads
 * nothing back); instead the kernel NEVER reads outside the arrays, in either validation mode: an entry index >= nnz or a column
 * >= n_cols contributes nothing and ORs into the validation word.
 * How (zkvm_pairings_amd/csrc/zkp_prove.hip, zkp_prove_plan.hpp): 2^t lanes (t = 0 .. 6, chosen on the host from nnz / n_rows) share a
 * row and stride its entries; adjacent lane groups take adjacent rows.  Values and vector entries stay canonical: mont_mul(val, x) is
 * val x / R, the lane sums add up, one more product with R^2 per output gives the canonical sum.  Exact; no atomics on field data.
 *
 * zkp_groth16_quotient_batch: out_h[j] = the N coefficients of h for witness j, in natural order, and out_sat[j].  ZKP_ERR_ARG, before
 * a byte is read: log2_n outside 1 .. 20, n_rows > N, the three matrices disagreeing on n_rows or n_cols, n_inputs + 1 > m, m > 2^22,
 * nnz > 2^31 - 1, n > 2^31 - 1, null pointers with non-zero counts; the host flavour checks the three matrices as above.  n == 0 is
 * legal; n_rows == 0 is legal and gives h = 0.
 * How: per slice, the product three times with stride N, three inverse NTTs, three forward coset NTTs, one pointwise kernel
 * a_i <- (a_i b_i - c_i) / (7^N - 1), one inverse coset NTT.  The evaluation side of every transform is bit-reversed, so none of the
 * seven needs a workspace.
 *
 * zkp_groth16_prove_batch: the n proofs.  The outputs are laid out as zkp_groth16_batch's a / inf_a / b / inf_b / c / inf_c, so they feed
 * the verifier unchanged; out_sat as above (a proof of an unsatisfied witness is still written; the verifier rejects it).  flags must
 * be 0.  ZKP_ERR_ARG as for the quotient, plus unknown flags.
 * How: shared-bases MSMs over the caller's witness rows (a_query, b_g1_query, b_g2_query, and a copy of l_query padded with
 * n_inputs + 1 leading infinite entries) and over the h rows (h_query padded with one infinite entry); the blinding terms through the
 * scalar multiplication and addition of zkp_g*_mul_batch / zkp_g*_add_batch.
 *
 * Slices and workspace.  The quotient and the prover run in slices of whole proofs, S = min(n, max(1, floor(2^22 / max(m, N)))) each,
 * so the context keeps (grow-only): quotient 64 B S N; prover 96 B S N + 97 B (m + N) + 1451 B S, each region rounded up to 256 B,
 * plus the MSM workspace of one slice (zkp_g1_msm_batch with shared_bases = 1, max(m, N) terms, S rows), the domain table and the
 * coset tables of zkp_fr_ntt_batch.
 */
#ifndef ZKP_PROVE_H
#define ZKP_PROVE_H

#include "zkp_pairings.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    size_t n_rows, n_cols, nnz;
    const void *row_ptr, *col, *val;                         /* n_rows + 1 u32, nnz u32, nnz x 4 u64 (canonical) */
} zkp_fr_csr;

typedef struct {
    unsigned log2_n;
    size_t n_inputs;
    zkp_fr_csr a, b, c;                                      /* the three share n_rows and n_cols = m */
} zkp_r1cs;

typedef struct {
    const void *alpha_g1, *beta_g1, *delta_g1, *beta_g2, *delta_g2;
    const void *a_query, *a_inf, *b_g1_query, *b_g1_inf, *b_g2_query, *b_g2_inf, *l_query, *l_inf, *h_query;
} zkp_groth16_pk;

int zkp_fr_spmv_batch(zkp_ctx* ctx, const zkp_fr_csr* mat, const uint64_t* x /* n x n_cols x 4 */, size_t n, size_t out_stride,
                      uint64_t* out /* n x out_stride x 4 */);
int zkp_fr_spmv_batch_dev(zkp_ctx* ctx, const zkp_fr_csr* mat, const void* d_x, size_t n, size_t out_stride, void* d_out, void* stream);

int zkp_groth16_quotient_batch(zkp_ctx* ctx, const zkp_r1cs* r1cs, const uint64_t* witness /* n x m x 4 */, size_t n,
                               uint64_t* out_h /* n x N x 4 */, uint8_t* out_sat /* n */);
int zkp_groth16_quotient_batch_dev(zkp_ctx* ctx, const zkp_r1cs* r1cs, const void* d_witness, size_t n, void* d_out_h, void* d_out_sat, void* stream);

int zkp_groth16_prove_batch(zkp_ctx* ctx, const zkp_r1cs* r1cs, const zkp_groth16_pk* pk, const uint64_t* witness /* n x m x 4 */,
                            const uint64_t* rs /* n x 2 x 4 */, size_t n, int flags /* 0 */, uint64_t* out_a /* n G1 */, uint8_t* out_inf_a,
                            uint64_t* out_b /* n G2 */, uint8_t* out_inf_b, uint64_t* out_c /* n G1 */, uint8_t* out_inf_c, uint8_t* out_sat /* n */);
int zkp_groth16_prove_batch_dev(zkp_ctx* ctx, const zkp_r1cs* r1cs, const zkp_groth16_pk* pk, const void* d_witness, const void* d_rs, size_t n, int flags,
                                void* d_out_a, void* d_out_inf_a, void* d_out_b, void* d_out_inf_b, void* d_out_c, void* d_out_inf_c, void* d_out_sat,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif
