/* Pure-C consumer of include/zkp_recover.h: no Python, no torch.  Build:
 *   gcc -O2 -I include integration/c/zkp_recover.c -L zkvm_pairings_amd -lzkp_pairings -Wl,-rpath,$PWD/zkvm_pairings_amd -o zkp_recover
 * A node that holds half the cells of a blob: f = X^3 with N = 4, extended to 8 points, cells of l = 2 - M = 4 cells in the stored
 * (bit-reversed) order.  Cells 1 and 2 are lost and their bytes overwritten.  Recover gives the coefficients back; the transform of the
 * coefficients gives all four cells; the cell producer - under the "ceremony" tau = 1, where every proof of X^3 is [tau] g1 = g - gives
 * all four proofs.  With three cells lost the blob is reported, not recovered. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zkp_recover.h"

int main(void) {
    zkp_ctx* ctx = NULL;
    int rc = zkp_init(0, &ctx);
    if (rc != ZKP_OK) { fprintf(stderr, "zkp_init: %s\n", zkp_strerror(rc)); return 2; }
    static const uint64_t g[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL,
                                   0x17f1d3a73197d794ULL, 0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL,
                                   0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    uint64_t padded[8][4], blob[8][4], held[8][4], coeffs[4][4], again[8][4];
    static const uint64_t f[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 0}};
    memset(padded, 0, sizeof padded);
    memcpy(padded, f, sizeof f);
    rc = zkp_fr_ntt_batch(ctx, &padded[0][0], 1, 3, ZKP_NTT_BITREV, &blob[0][0]);
    if (rc != ZKP_OK) { fprintf(stderr, "extend: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 3; }
    /* cell m is entries 2 m and 2 m + 1 of the extended blob */
    uint8_t present[4] = {1, 0, 0, 1};
    int32_t ok = -1;
    memcpy(held, blob, sizeof blob);
    memset((unsigned char*)held + 2 * sizeof held[0], 0xff, 4 * sizeof held[0]);
    rc = zkp_das_recover_batch(ctx, &held[0][0], present, 1, 2, 1, ZKP_NTT_BITREV, &coeffs[0][0], &ok);
    if (rc != ZKP_OK || ok != 1) { fprintf(stderr, "recover: rc %d ok %d (%s)\n", rc, (int)ok, zkp_last_error(ctx)); return 4; }
    if (memcmp(coeffs, f, sizeof f)) { fprintf(stderr, "the recovered coefficients are not those of X^3\n"); return 5; }
    /* all the cells: the transform of the recovered coefficients, zero-padded to D */
    memset(padded, 0, sizeof padded);
    memcpy(padded, coeffs, sizeof coeffs);
    rc = zkp_fr_ntt_batch(ctx, &padded[0][0], 1, 3, ZKP_NTT_BITREV, &again[0][0]);
    if (rc != ZKP_OK || memcmp(again, blob, sizeof blob)) { fprintf(stderr, "the cells of the recovered polynomial differ: rc %d\n", rc); return 6; }
    /* all the proofs */
    uint64_t mono[4][12], setup[8][12], proof[4][12];
    uint8_t setup_inf[8], proof_inf[4];
    for (int i = 0; i < 4; i++) memcpy(mono[i], g, sizeof g);
    rc = zkp_kzg_cells_setup(ctx, &mono[0][0], 2, 1, &setup[0][0], setup_inf);
    if (rc != ZKP_OK) { fprintf(stderr, "cells setup: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 7; }
    rc = zkp_kzg_cells_batch(ctx, &setup[0][0], setup_inf, &coeffs[0][0], 1, 2, 1, 1, ZKP_NTT_BITREV, &proof[0][0], proof_inf);
    if (rc != ZKP_OK) { fprintf(stderr, "cells: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 8; }
    for (int i = 0; i < 4; i++)
        if (proof_inf[i] || memcmp(proof[i], g, sizeof g)) { fprintf(stderr, "proof %d of the recovered X^3 is not [tau] g1\n", i); return 9; }
    /* one cell is not enough: reported, a zero row, no error status */
    present[3] = 0;
    rc = zkp_das_recover_batch(ctx, &held[0][0], present, 1, 2, 1, ZKP_NTT_BITREV, &coeffs[0][0], &ok);
    memset(padded, 0, sizeof padded);
    if (rc != ZKP_OK || ok != 0 || memcmp(coeffs, padded, sizeof coeffs)) { fprintf(stderr, "one cell of four: rc %d ok %d\n", rc, (int)ok); return 10; }
    if (zkp_das_recover_batch(ctx, &held[0][0], present, 1, 11, 0, 0, &coeffs[0][0], &ok) != ZKP_ERR_ARG) {
        fprintf(stderr, "a column of 4096 cells was accepted\n");
        return 11;
    }
    printf("zkp_recover ok: X^3 back from two of four cells, its cells and four proofs rebuilt, one cell of four reported\n");
    zkp_free(ctx);
    return 0;
}
