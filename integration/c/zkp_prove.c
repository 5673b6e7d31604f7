/* Pure-C consumer of include/zkp_prove.h: no Python, no torch.  Build:
 *   gcc -O2 -I include integration/c/zkp_prove.c -L zkvm_pairings_amd -lzkp_pairings -Wl,-rpath,$PWD/zkvm_pairings_amd -o zkp_prove
 * The circuit "x * x = y" over the two-point domain: variables (1, x, y), row 0: z1 * z1 = z2, row 1: z0 * z2 = z2.  Multiplies the
 * A matrix with two witnesses (zkp_fr_spmv_batch), then asks for their quotients (zkp_groth16_quotient_batch): (1, 3, 9) satisfies
 * the system and its quotient has degree 0, (1, 3, 10) does not. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zkp_prove.h"

int main(void) {
    zkp_ctx* ctx = NULL;
    int rc = zkp_init(0, &ctx);
    if (rc != ZKP_OK) { fprintf(stderr, "zkp_init: %s\n", zkp_strerror(rc)); return 2; }
    static const uint32_t a_ptr[3] = {0, 1, 2}, a_col[2] = {1, 0};
    static const uint32_t b_ptr[3] = {0, 1, 2}, b_col[2] = {1, 2};
    static const uint32_t c_ptr[3] = {0, 1, 2}, c_col[2] = {2, 2};
    static const uint64_t ones[8] = {1, 0, 0, 0, 1, 0, 0, 0};
    static const uint64_t witness[2][3][4] = {{{1, 0, 0, 0}, {3, 0, 0, 0}, {9, 0, 0, 0}}, {{1, 0, 0, 0}, {3, 0, 0, 0}, {10, 0, 0, 0}}};
    zkp_r1cs sys;
    memset(&sys, 0, sizeof sys);
    sys.log2_n = 1;
    sys.n_inputs = 1;
    sys.a.n_rows = sys.b.n_rows = sys.c.n_rows = 2;
    sys.a.n_cols = sys.b.n_cols = sys.c.n_cols = 3;
    sys.a.nnz = sys.b.nnz = sys.c.nnz = 2;
    sys.a.row_ptr = a_ptr; sys.a.col = a_col; sys.a.val = ones;
    sys.b.row_ptr = b_ptr; sys.b.col = b_col; sys.b.val = ones;
    sys.c.row_ptr = c_ptr; sys.c.col = c_col; sys.c.val = ones;
    uint64_t az[2][2][4];
    rc = zkp_fr_spmv_batch(ctx, &sys.a, &witness[0][0][0], 2, 2, &az[0][0][0]);
    if (rc != ZKP_OK) { fprintf(stderr, "spmv: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 3; }
    for (int j = 0; j < 2; j++)
        if (az[j][0][0] != 3 || az[j][1][0] != 1 || az[j][0][1] || az[j][1][3]) { fprintf(stderr, "A z is wrong for witness %d\n", j); return 4; }
    uint64_t h[2][2][4];
    uint8_t sat[2] = {9, 9};
    rc = zkp_groth16_quotient_batch(ctx, &sys, &witness[0][0][0], 2, &h[0][0][0], sat);
    if (rc != ZKP_OK) { fprintf(stderr, "quotient: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 5; }
    if (sat[0] != 1 || sat[1] != 0) { fprintf(stderr, "sat = %d %d\n", sat[0], sat[1]); return 6; }
    for (int w = 0; w < 4; w++)
        if (h[0][1][w]) { fprintf(stderr, "the quotient of a satisfying witness has degree N - 1\n"); return 7; }
    sys.b.n_cols = 4;   /* the three matrices must agree */
    if (zkp_groth16_quotient_batch(ctx, &sys, &witness[0][0][0], 2, &h[0][0][0], sat) != ZKP_ERR_ARG) { fprintf(stderr, "shape mismatch accepted\n"); return 8; }
    printf("zkp_prove ok: A z = (3, 1), sat = (1, 0), h_0 = 0x%016llx...\n", (unsigned long long)h[0][0][3]);
    zkp_free(ctx);
    return 0;
}
