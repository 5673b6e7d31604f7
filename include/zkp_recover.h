/*
 * include/zkp_recover.h -- the recovery layer of libzkp_pairings.so: erased blobs back from any half of their cells, the third operation
 * of a data-availability node beside the cell producer and the cell verifier.  A sixth header of the SAME library: include it beside
 * zkp_cells.h, whose contract and notation it shares - zkp_pairings.h's zkp_ctx, zkp_status codes, zkp_set_validate and validation word
 * (zkp_take_validation_status_dev), zkp_poly.h's ZKP_NTT_BITREV and root of unity.  Symbols added under ABI version 4 (zkp_abi_version()
 * is still 4).  Fr work only: no group element and no pairing is touched.
 *
 * The entry point has a host-pointer flavour and a _dev flavour with a trailing stream.  The _dev flavour is asynchronous, reads nothing
 * back, and is capturable into a hipGraph once the context's workspace and tables have reached the call's size (run the call once before
 * capturing it) - the contract of zkp_fr_eval_batch_dev.
 *
 * Sizes, as in zkp_cells.h with the extension fixed at 2: N = 2^log2_n coefficients per polynomial f, cells of l = 2^log2_l values, D = 2 N
 * points, M = D / l cells, k = N / l = M / 2.  Cell m is the coset c_m H_l with c_m = w_D^m' - m' = bitrev_M(m) under ZKP_NTT_BITREV, m
 * otherwise - and its value u is f(c_m w_l^u'), u' = bitrev_l(u) under the flag: the order of zkp_kzg_cells_batch and of
 * zkp_kzg_cell_verify_batch.
 *
 * zkp_das_recover_batch: n extended blobs in cell order (values: n x M x l x 4 words, cell m of blob j is row [j][m]) with a mask
 * (present[j][m] != 0: the cell was received).  The bytes of a missing cell are never interpreted: they may be anything, values >= r
 * included.  out_coeffs row j is f_j in COEFFICIENT form, canonical - the input of zkp_kzg_cells_batch and, zero-padded to D, of
 * zkp_fr_ntt_batch.  out_ok[j] = 1 iff at least M / 2 cells of blob j are present and they are consistent with a polynomial of degree
 * below N.  Fewer than M / 2 present cells: the row is all zero and ok = 0.  Inconsistent cells: ok = 0 and the row is unspecified but
 * canonical.  Exactly M / 2 present cells: any data is consistent, ok = 1 and the row is the unique interpolant.  Neither case is an error
 * status.  In validation mode the values of PRESENT cells are checked: one >= r gives ZKP_ERR_NONCANONICAL on the host flavour and ORs
 * into the validation word on the _dev one.
 * ZKP_ERR_ARG, before a byte is read: log2_n > 19, log2_l > log2_n, log2_n + 1 - log2_l > 10 (M <= 1024: a column must fit the kernel's
 * LDS tile), n D > 2^26, flags other than ZKP_NTT_BITREV, null pointers with a non-zero count; n == 0 is legal.
 * How (zkvm_pairings_amd/csrc/zkp_recover.hip, zkp_recover_plan.hpp): write f(X) = sum_{i<l} X^i P_i(X^l), P_i of degree below k.  The
 * interpolant of cell m is f mod (X^l - c_m^l) = sum_i X^i P_i(w_M^m'), w_M = w_D^l: the inverse Fr transform of size l over the cells,
 * coefficient i times c_m^-i (the domain table) - what the cell verifier computes.  Across cells, column i of those coefficients is the
 * Reed-Solomon codeword of P_i on the M-th roots of unity, so a blob is l independent erasure decodings of size M with ONE erasure
 * pattern: Z(Y) = prod over the missing m' of (Y - w_M^m'), degree at most M / 2, is shared by the columns.  k_rec_vanish, a workgroup per
 * blob, counts the present cells and multiplies Z up in LDS one linear factor at a time; two Fr transforms of size M give Z on the M-th
 * roots and on the coset 7 w_M^t (7 has order r - 1: no zero there).  k_rec_zinv, a workgroup per blob, inverts the second table in place
 * WITHOUT a field inversion: prod_t Z(7 w_M^t) = (1 - 7^M)^deg Z, so Montgomery's trick starts from a known total - a power of a constant
 * of the call - and is two prefix-product scans in LDS.  Then ONE kernel, k_rec_column, a workgroup per C = min(l, 1024 / M) consecutive
 * columns of a blob, everything in a 32 KiB LDS tile: E[m'] Z(w_M^m') on load (0 for a missing cell, unread), the inverse transform
 * (P_i Z), the forward transform on the coset, the product with 1 / Z, the inverse coset transform: p.  f_{i + l t} = p_t for t < k, and
 * the cells are consistent iff p_t = 0 for every t >= k in every column.
 * Cost: two passes over the data - n D elements read and written by the size-l transform, read once more and n N written by the
 * column kernel - and 3 (M / 2) log2 M + 5 M products per column, against three transforms of size D and about eight passes of the
 * textbook decoder.  Per blob at most M / 2 dependent steps build Z (64 at N = 4096, l = 64; 512 at M = 1024) and 2 log2 M invert its table:
 * the latency of a small call.  Exact; no atomics.
 * Slices and workspace: slices of whole blobs, floor(2^21 / D) each (at least one).  Per blob of a slice D field elements (32 B; none
 * for l = 1, as many again for a natural-order transform with l > 1024) and 3 M more: 64 MiB + 3 MiB at N = 4096, l = 64.  The workspace
 * is the one of zkp_fr_invert_batch, zkp_fr_eval_batch and the two KZG verifiers, grow-only, as are the domain table of D points and the
 * coset tables.
 */
#ifndef ZKP_RECOVER_H
#define ZKP_RECOVER_H

#include "zkp_cells.h"

#ifdef __cplusplus
extern "C" {
#endif

int zkp_das_recover_batch(zkp_ctx* ctx, const uint64_t* values /* n x M x l x 4 */, const uint8_t* present /* n x M */, size_t n, unsigned log2_n,
                          unsigned log2_l, int flags /* ZKP_NTT_BITREV or 0 */, uint64_t* out_coeffs /* n x N x 4 */, int32_t* out_ok /* n */);
int zkp_das_recover_batch_dev(zkp_ctx* ctx, const void* d_values, const void* d_present, size_t n, unsigned log2_n, unsigned log2_l, int flags,
                              void* d_out_coeffs, void* d_out_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif
