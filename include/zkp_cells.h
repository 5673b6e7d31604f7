/*
 * include/zkp_cells.h -- the cell layer of libzkp_pairings.so: KZG proofs of a polynomial on whole cosets of its extended domain
 * ("cells", the unit a data-availability producer publishes) by the Feist-Khovratovich multi-proof method, and a batch verifier for
 * them.  A fifth header of the SAME library: include it beside zkp_fk20.h, whose contract it shares - zkp_pairings.h's zkp_ctx,
 * zkp_status codes, zkp_set_validate, validation word (zkp_take_validation_status_dev) and wire formats, zkp_poly.h's ZKP_NTT_* flags
 * and root of unity.  Symbols added under ABI version 4 (zkp_abi_version() is still 4).
 *
 * Each entry point has a host-pointer flavour and a _dev flavour with a trailing stream.  The _dev flavour is asynchronous, reads
 * nothing back, and is capturable into a hipGraph once the context's workspaces and tables have reached the call's size (run the call
 * once before capturing it) - the contract of zkp_fr_eval_batch_dev.  G1 points are 12 words (x, y), the identity is (0, 1) with its flag
 * set, like every group output.  The producer's input points are TRUSTED: on the curve and in the subgroup, the contract of the MSM; a
 * producer checks its setup once with zkp_g1_is_valid_batch.  In validation mode a coordinate >= p or a field element >= r gives
 * ZKP_ERR_NONCANONICAL on the host flavour and ORs into the validation word on the _dev one.
 *
 * Sizes.  N = 2^log2_n coefficients per polynomial f; cells of l = 2^log2_l values, l <= N, k = N / l; an extension e = 2^log2_ext,
 * log2_ext 0 or 1; D = e N points, M = D / l cells.  w_D is the root of zkp_fr_ntt_batch at size D, w_l = w_D^M.  Cell m is the coset
 * c_m H_l with c_m = w_D^m' - m' = bitrev_M(m) under ZKP_NTT_BITREV, m otherwise - and its value u is f(c_m w_l^u'), u' = bitrev_l(u)
 * under ZKP_NTT_BITREV, u otherwise.  Under ZKP_NTT_BITREV the M x l values of a polynomial, row-major, are exactly zkp_fr_ntt_batch
 * with ZKP_NTT_BITREV of its coefficients zero-padded to D: cell m is entries [l m, l m + l) of the bit-reversed extended blob.  The
 * values are therefore not an output of the producer.  Proof m is [q_m(tau)] g1 for q_m = (f - I_m) / (X^l - c_m^l), I_m = f mod
 * (X^l - c_m^l): the polynomial of degree below l that agrees with f on the coset.  l = 1 is the single proof of zkp_kzg_fk20_batch;
 * for l = N every proof is the identity.  Cell (C, m, v_0 .. v_{l-1}, pi) holds iff
 *     e(C - [I(tau)] g1 + [c_m^l] pi, g2) = e(pi, [tau^l] g2),   I the interpolant of the l values on the coset.
 *
 * zkp_kzg_cells_setup: from the monomial setup monomial_g1[k] = [tau^k] g1, k < N, the 2 N points the proofs need, as l vectors of 2 k
 * points, out[i][t]: vector i is the forward G1 NTT of size 2 k (natural order) of (s_{N-l-1-i}, s_{N-2l-1-i}, ..) - k - 1 points, the
 * setup index stepping down by l - followed by k + 1 identities.  Computed once per setup and cell size.  For l = 1 the output is
 * zkp_kzg_fk20_setup's byte for byte; for l = N it is 2 N identities.  ZKP_ERR_ARG: log2_n > 19, log2_l > log2_n, null pointers.
 *
 * zkp_kzg_cells_batch: n polynomials in COEFFICIENT form (n x N x 4 words, canonical) against the output of zkp_kzg_cells_setup for the
 * same log2_n and log2_l (cells_setup_inf may be NULL: every point finite).  out_proof[j][m] is proof m of polynomial j as defined
 * above, n x M points.  Each proof is what zkp_kzg_cell_verify_batch consumes.  ZKP_ERR_ARG, before a byte is read: log2_n > 19,
 * log2_l > log2_n, log2_ext > 1, n N > 2^21, flags other than ZKP_NTT_BITREV, null pointers with a non-zero count; n == 0 is legal.
 * How, per polynomial (zkvm_pairings_amd/csrc/zkp_cells.hip, zkp_coop.hip, zkp_cells_plan.hpp): for every stride i < l the vector
 * c_i = (f_{N-1-i}, 0 x (k + 1), f_{2l-1-i}, .., f_{N-l-1-i}) / (2 k); ONE batched Fr transform of size 2 k over the l vectors; slot by
 * slot H[t] = sum_i [c^_i[t]] X_i[t] - the l bases of a slot are summed anyway, so a lane takes g = 2^s consecutive strides of a slot
 * through ONE chain of 255 doublings, adding each base whose scalar has the bit (mixed addition, every exceptional case), and a second
 * kernel adds the l / g partials of a slot by the full addition; the inverse G1 transform of size 2 k, unscaled - its first k entries
 * are h, entry k - 1 the identity by construction; the forward G1 transform of size M of h padded with identities is the M proofs.  g
 * is chosen per call from the lane count, 2 N lanes per polynomial of a slice at g = 1: g = 1 while those leave SIMDs idle (up to 2^16:
 * the shortest chain wins), then the smallest of 2, 4 that brings the lanes back to one wavefront per SIMD, never above l.
 * Cost: 2 N mixed-addition chains sharing 2 N / g chains of 255 doublings, and about (k + M / 2) log2 k 128-bit scalar multiplications
 * in the transforms, against FK20's 2 N 255-bit and (3 N / 2) log2 N 128-bit ones.  Exact; no atomics.
 * Slices and workspace: slices of whole polynomials, floor(2^17 / N) each (at least one).  Per polynomial of a slice 2 N field elements
 * (32 B), 2 M Jacobian records (192 B; 2 M <= 4 N / l) and, unless g = l, 2 N / g partial records: at most 2^18 of each up to N = 2^17 -
 * 8 MiB, 96 MiB (l = 1, e = 2: 2^19 records) and 48 MiB - and 2 N, 4 N / l and 2 N / g of them beyond.  The workspace is the one of
 * zkp_g1_ntt_batch and zkp_kzg_fk20_batch, grow-only, as are the domain table and the split twiddles of 2 k points.
 *
 * zkp_kzg_cell_verify_batch: n cells against ONE setup - monomial_g1_l[i] = [tau^i] g1 for i < l, g2, tau_l_g2 = [tau^l] g2 - each
 * cell with a commitment of its own (repeats allowed), its index cell_index[j] < M = 2^(log2_d - log2_l), its l values (n x l x 4 words,
 * in-cell order by the flag) and its proof.  rand: n pairs (a, b) of 64-bit words exactly as for zkp_kzg_verify_batch, r_j = a_j +
 * b_j z^2.  *out_ok = 1 iff
 *     e(sum r_j pi_j, [tau^l] g2) = e(sum r_j C_j - [sum_j r_j I_j(tau)] g1 + sum r_j c_j^l pi_j, g2)
 * and every point is valid, every value < r, every index < M and no (a_j, b_j) is zero; a batch with n == 0 passes.  flags:
 * ZKP_NTT_BITREV (order of the cells and of their values), ZKP_CELLS_POINTS_CHECKED (commitments and proofs are known to be valid
 * points), ZKP_CELLS_VK_CHECKED (the l + 1 setup points and the two G2 points are); without them is_valid runs over those points as
 * in zkp_kzg_verify_batch.  ZKP_ERR_ARG: log2_d > 20, log2_l > log2_d, log2_l > 15 (the fold's width), n > 2^21, n l > 2^26, unknown
 * flags, null pointers (inf_c and inf_proof may be NULL; with n == 0 only ctx and out_ok are looked at).
 * How: the inverse Fr transform of size l over the n value rows; k_cell_scale multiplies coefficient i of row j by c_j^-i =
 * w_D^(-(m' i) mod D), read from the cached domain table of D points, and writes r_j and r_j c_j^l; fr_fold over j leaves the l
 * coefficients of sum_j r_j I_j; ONE shared-bases MSM call over the 2 n + l points C | pi | monomial, rows r | r c^l | -coefficients and
 * 0 | r | 0; one Miller product over the two pairs, one final exponentiation.  Workspace: about 32 (n l + 6 n + 2 l) B + 97 (2 n + l) B
 * of the verifier's grow-only workspace, beside the MSM's.
 */
#ifndef ZKP_CELLS_H
#define ZKP_CELLS_H

#include "zkp_fk20.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKP_CELLS_POINTS_CHECKED 4
#define ZKP_CELLS_VK_CHECKED 8

int zkp_kzg_cells_setup(zkp_ctx* ctx, const uint64_t* monomial_g1 /* N finite G1 points */, unsigned log2_n, unsigned log2_l, uint64_t* out /* l x 2k G1 */,
                        uint8_t* out_inf /* 2N */);
int zkp_kzg_cells_setup_dev(zkp_ctx* ctx, const void* d_monomial_g1, unsigned log2_n, unsigned log2_l, void* d_out, void* d_out_inf, void* stream);

int zkp_kzg_cells_batch(zkp_ctx* ctx, const uint64_t* cells_setup /* 2N G1 */, const uint8_t* cells_setup_inf /* 2N, may be NULL */,
                        const uint64_t* coeffs /* n x N x 4 */, size_t n, unsigned log2_n, unsigned log2_l, unsigned log2_ext,
                        int flags /* ZKP_NTT_BITREV or 0 */, uint64_t* out_proof /* n x M G1 */, uint8_t* out_inf /* n x M */);
int zkp_kzg_cells_batch_dev(zkp_ctx* ctx, const void* d_cells_setup, const void* d_cells_setup_inf, const void* d_coeffs, size_t n, unsigned log2_n,
                            unsigned log2_l, unsigned log2_ext, int flags, void* d_out_proof, void* d_out_inf, void* stream);

int zkp_kzg_cell_verify_batch(zkp_ctx* ctx, const uint64_t* monomial_g1_l /* l G1 */, const uint64_t* g2, const uint64_t* tau_l_g2,
                              const uint64_t* commitments /* n G1 */, const uint8_t* inf_c /* n, may be NULL */, const uint32_t* cell_index /* n */,
                              const uint64_t* values /* n x l x 4 */, const uint64_t* proofs /* n G1 */, const uint8_t* inf_proof /* n, may be NULL */,
                              size_t n, unsigned log2_d, unsigned log2_l, int flags, const uint64_t* rand /* n x 2 */, int* out_ok);
int zkp_kzg_cell_verify_batch_dev(zkp_ctx* ctx, const void* d_monomial_g1_l, const void* d_g2, const void* d_tau_l_g2, const void* d_commitments,
                                  const void* d_inf_c, const void* d_cell_index, const void* d_values, const void* d_proofs, const void* d_inf_proof, size_t n,
                                  unsigned log2_d, unsigned log2_l, int flags, const void* d_rand, void* d_out_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif
