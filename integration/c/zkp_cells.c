/* Pure-C consumer of include/zkp_cells.h: no Python, no torch.  Build:
 *   gcc -O2 -I include integration/c/zkp_cells.c -L zkvm_pairings_amd -lzkp_pairings -Wl,-rpath,$PWD/zkvm_pairings_amd -o zkp_cells
 * The "ceremony" tau = 1: every monomial point is the generator and [tau^l] g2 = g2.  f = X^3 with N = 4, cells of l = 2 on the domain of
 * 8 points: X^3 = X (X^2 - a) + a X, so every one of the M = 4 proofs is [tau] g1 = g.  Then the verifier on two cells of the zero
 * polynomial - identity commitment, zero values, identity proof - which hold, and stop holding once a value is one. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zkp_cells.h"

int main(void) {
    zkp_ctx* ctx = NULL;
    int rc = zkp_init(0, &ctx);
    if (rc != ZKP_OK) { fprintf(stderr, "zkp_init: %s\n", zkp_strerror(rc)); return 2; }
    /* the generators of G1 and G2, little-endian 64-bit words */
    static const uint64_t g[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL,
                                   0x17f1d3a73197d794ULL, 0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL,
                                   0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    static const uint64_t g2[24] = {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL,
                                    0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL, 0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL,
                                    0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL,
                                    0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL,
                                    0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL, 0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL,
                                    0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
    uint64_t mono[4][12], setup[8][12], proof[4][12];
    uint8_t setup_inf[8], proof_inf[4];
    static const uint64_t coeffs[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 0}};
    for (int i = 0; i < 4; i++) memcpy(mono[i], g, sizeof g);
    rc = zkp_kzg_cells_setup(ctx, &mono[0][0], 2, 1, &setup[0][0], setup_inf);
    if (rc != ZKP_OK) { fprintf(stderr, "cells setup: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 3; }
    rc = zkp_kzg_cells_batch(ctx, &setup[0][0], setup_inf, &coeffs[0][0], 1, 2, 1, 1, ZKP_NTT_BITREV, &proof[0][0], proof_inf);
    if (rc != ZKP_OK) { fprintf(stderr, "cells: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 4; }
    for (int i = 0; i < 4; i++)
        if (proof_inf[i] || memcmp(proof[i], g, sizeof g)) { fprintf(stderr, "proof %d of X^3 is not [tau] g1\n", i); return 5; }
    if (zkp_kzg_cells_batch(ctx, &setup[0][0], setup_inf, &coeffs[0][0], 1, 2, 3, 1, 0, &proof[0][0], proof_inf) != ZKP_ERR_ARG) {
        fprintf(stderr, "a cell larger than the polynomial was accepted\n");
        return 6;
    }
    uint64_t com[2][12], pi[2][12], values[2][2][4];
    uint8_t inf[2] = {1, 1};
    static const uint32_t index[2] = {0, 3};
    static const uint64_t rand[2][2] = {{0x9e3779b97f4a7c15ULL, 1}, {3, 0xbf58476d1ce4e5b9ULL}};
    memset(com, 0, sizeof com);
    memset(values, 0, sizeof values);
    com[0][6] = com[1][6] = 1;
    memcpy(pi, com, sizeof com);
    int ok = -1;
    rc = zkp_kzg_cell_verify_batch(ctx, &mono[0][0], g2, g2, &com[0][0], inf, index, &values[0][0][0], &pi[0][0], inf, 2, 3, 1, ZKP_NTT_BITREV, &rand[0][0], &ok);
    if (rc != ZKP_OK || ok != 1) { fprintf(stderr, "two cells of the zero polynomial: rc %d ok %d (%s)\n", rc, ok, zkp_last_error(ctx)); return 7; }
    values[1][1][0] = 1;
    rc = zkp_kzg_cell_verify_batch(ctx, &mono[0][0], g2, g2, &com[0][0], inf, index, &values[0][0][0], &pi[0][0], inf, 2, 3, 1, ZKP_NTT_BITREV, &rand[0][0], &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "a changed value: rc %d ok %d\n", rc, ok); return 8; }
    printf("zkp_cells ok: four proofs of X^3 equal [tau] g1, two cells verified, one changed value refused\n");
    zkp_free(ctx);
    return 0;
}
