/* Pure-C consumer of include/zkp_fk20.h: no Python, no torch.  Build:
 *   gcc -O2 -I include integration/c/zkp_fk20.c -L zkvm_pairings_amd -lzkp_pairings -Wl,-rpath,$PWD/zkvm_pairings_amd -o zkp_fk20
 * A vector of four points - the generator and three identities - has the constant transform (g, g, g, g); transforming that forward
 * again and inverting brings it back.  Then the FK20 setup of the "ceremony" tau = 1 (every monomial point is the generator) and the
 * proofs of the constant polynomial 5, which are all infinite. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zkp_fk20.h"

int main(void) {
    zkp_ctx* ctx = NULL;
    int rc = zkp_init(0, &ctx);
    if (rc != ZKP_OK) { fprintf(stderr, "zkp_init: %s\n", zkp_strerror(rc)); return 2; }
    /* the generator of G1, little-endian 64-bit words of x then y */
    static const uint64_t g[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL,
                                   0x17f1d3a73197d794ULL, 0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL,
                                   0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    uint64_t v[4][12], out[4][12], back[4][12];
    uint8_t inf[4] = {0, 1, 1, 1}, out_inf[4], back_inf[4];
    memset(v, 0, sizeof v);
    memcpy(v[0], g, sizeof g);
    for (int i = 1; i < 4; i++) v[i][6] = 1;
    rc = zkp_g1_ntt_batch(ctx, &v[0][0], inf, 1, 2, 0, &out[0][0], out_inf);
    if (rc != ZKP_OK) { fprintf(stderr, "g1 ntt: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 3; }
    for (int i = 0; i < 4; i++)
        if (out_inf[i] || memcmp(out[i], g, sizeof g)) { fprintf(stderr, "the transform of (g, 0, 0, 0) is not constant at %d\n", i); return 4; }
    rc = zkp_g1_ntt_batch(ctx, &out[0][0], out_inf, 1, 2, ZKP_NTT_INVERSE, &back[0][0], back_inf);
    if (rc != ZKP_OK) { fprintf(stderr, "g1 intt: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 5; }
    if (memcmp(back, v, sizeof v) || memcmp(back_inf, inf, sizeof inf)) { fprintf(stderr, "the inverse does not give the input back\n"); return 6; }
    if (zkp_g1_ntt_batch(ctx, &v[0][0], inf, 1, 2, ZKP_NTT_COSET, &out[0][0], out_inf) != ZKP_ERR_ARG) { fprintf(stderr, "coset accepted\n"); return 7; }
    uint64_t mono[4][12], setup[8][12], proof[4][12];
    uint8_t setup_inf[8], proof_inf[4];
    static const uint64_t coeffs[4][4] = {{5, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int i = 0; i < 4; i++) memcpy(mono[i], g, sizeof g);
    rc = zkp_kzg_fk20_setup(ctx, &mono[0][0], 2, &setup[0][0], setup_inf);
    if (rc != ZKP_OK) { fprintf(stderr, "fk20 setup: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 8; }
    rc = zkp_kzg_fk20_batch(ctx, &setup[0][0], setup_inf, &coeffs[0][0], 1, 2, ZKP_NTT_BITREV, &proof[0][0], proof_inf);
    if (rc != ZKP_OK) { fprintf(stderr, "fk20: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 9; }
    for (int i = 0; i < 4; i++)
        if (!proof_inf[i] || proof[i][0] || proof[i][6] != 1) { fprintf(stderr, "a constant polynomial has a finite proof at %d\n", i); return 10; }
    printf("zkp_fk20 ok: NTT(g, 0, 0, 0) = (g, g, g, g), inverse exact, four infinite proofs of a constant\n");
    zkp_free(ctx);
    return 0;
}
