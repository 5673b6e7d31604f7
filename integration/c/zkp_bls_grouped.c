/* Pure-C consumer of include/zkp_bls_grouped.h: no Python, no torch.  Build:
 *   gcc -O2 -I include integration/c/zkp_bls_grouped.c -L zkvm_pairings_amd -lzkp_pairings -Wl,-rpath,$PWD/zkvm_pairings_amd -o zkp_bls_grouped
 * Three validators with the secret keys 3, 5 and 9; the first two sign "abc", the third signs "xyz".  The scaled sum of the first group
 * under (a, b) = (2, 0) and (1, 0) must be [2 * 3 + 5] g1 = [11] g1; the three signatures ordered by message verify with two hashes and
 * three Miller loops; with the two signatures of "abc" swapped they do not; offsets that do not end at the number of signatures are
 * refused. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zkp_bls_grouped.h"

int main(void) {
    zkp_ctx* ctx = NULL;
    int rc = zkp_init(0, &ctx);
    if (rc != ZKP_OK) { fprintf(stderr, "zkp_init: %s\n", zkp_strerror(rc)); return 2; }
    static const uint64_t g[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL,
                                   0x17f1d3a73197d794ULL, 0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL,
                                   0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    static const char eth_dst[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
    /* rows 0..2: the validators' keys; row 3: [11] g1, to compare with */
    const uint64_t sk[4][4] = {{3, 0, 0, 0}, {5, 0, 0, 0}, {9, 0, 0, 0}, {11, 0, 0, 0}};
    uint64_t pk[4 * 12];
    uint8_t pinf[4];
    rc = zkp_g1_mul_batch(ctx, g, 0, &sk[0][0], 4, pk, pinf);
    if (rc != ZKP_OK) { fprintf(stderr, "keys: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 3; }
    const uint64_t grp_off[3] = {0, 2, 3};
    const uint64_t small[6] = {2, 0, 1, 0, 7, 0};
    uint64_t sum[2 * 12];
    uint8_t sinf[2], st[2];
    rc = zkp_g1_scaled_segment_sum_batch(ctx, pk, NULL, small, 3, grp_off, 2, sum, sinf, st);
    if (rc != ZKP_OK) { fprintf(stderr, "scaled sums: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 4; }
    if (memcmp(sum, pk + 36, 96) || sinf[0] || sinf[1] || st[0] || st[1]) {
        fprintf(stderr, "[2] pk_0 + [1] pk_1 is not [11] g1\n");
        return 5;
    }
    /* the two distinct messages, hashed once each to sign with */
    const uint8_t msgs[6] = {'a', 'b', 'c', 'x', 'y', 'z'};
    const uint64_t offsets[3] = {0, 3, 6};
    uint64_t hm[2 * 24], base[3 * 24], sig[3 * 24], swapped[3 * 24];
    uint8_t hinf[2], sig_inf[3];
    rc = zkp_hash_to_g2_batch(ctx, msgs, offsets, 2, (const uint8_t*)eth_dst, strlen(eth_dst), hm, hinf);
    memcpy(base, hm, 192);
    memcpy(base + 24, hm, 192);
    memcpy(base + 48, hm + 24, 192);
    if (rc == ZKP_OK) rc = zkp_g2_mul_batch(ctx, base, 24, &sk[0][0], 3, sig, sig_inf);
    if (rc != ZKP_OK || hinf[0] || hinf[1] || sig_inf[0] || sig_inf[1] || sig_inf[2]) {
        fprintf(stderr, "sign: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx));
        return 6;
    }
    const uint64_t rnd[6] = {0x9e3779b97f4a7c15ULL, 0xbf58476d1ce4e5b9ULL, 0x94d049bb133111ebULL, 0x2545f4914f6cdd1dULL, 0xd6e8feb86659fd93ULL, 0x1ULL};
    int ok = -1;
    rc = zkp_bls_verify_grouped_batch(ctx, pk, NULL, grp_off, msgs, offsets, 2, (const uint8_t*)eth_dst, strlen(eth_dst), sig, NULL, 3, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 1) { fprintf(stderr, "verify: rc %d ok %d (%s)\n", rc, ok, zkp_last_error(ctx)); return 7; }
    memcpy(swapped, sig + 24, 192);
    memcpy(swapped + 24, sig, 192);
    memcpy(swapped + 48, sig + 48, 192);
    rc = zkp_bls_verify_grouped_batch(ctx, pk, NULL, grp_off, msgs, offsets, 2, (const uint8_t*)eth_dst, strlen(eth_dst), swapped, NULL, 3, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "two swapped signatures of one message verified: rc %d ok %d\n", rc, ok); return 8; }
    const uint64_t short_off[3] = {0, 2, 2};
    if (zkp_bls_verify_grouped_batch(ctx, pk, NULL, short_off, msgs, offsets, 2, (const uint8_t*)eth_dst, strlen(eth_dst), sig, NULL, 3, rnd, 0, &ok) !=
        ZKP_ERR_ARG) {
        fprintf(stderr, "offsets that stop before the last signature were accepted\n");
        return 9;
    }
    printf("zkp_bls_grouped ok: the scaled sum is [11] g1, three signatures over two messages verified, a swapped pair refused\n");
    zkp_free(ctx);
    return 0;
}
