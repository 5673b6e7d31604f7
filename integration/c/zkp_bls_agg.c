/* Pure-C consumer of include/zkp_bls_agg.h: no Python, no torch.  Build:
 *   gcc -O2 -I include integration/c/zkp_bls_agg.c -L zkvm_pairings_amd -lzkp_pairings -Wl,-rpath,$PWD/zkvm_pairings_amd -o zkp_bls_agg
 * Three validators with the secret keys 3, 5 and 9 in a table with their total as a fourth row.  The committee {0, 2} must sum to
 * [12] g1 and "the total minus validator 1" to the same point; the aggregate signature [12] H(m) verifies under the committee, not under
 * the committee {0, 1}; an empty committee does not verify; offsets that do not end at the number of entries are refused. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zkp_bls_agg.h"

int main(void) {
    zkp_ctx* ctx = NULL;
    int rc = zkp_init(0, &ctx);
    if (rc != ZKP_OK) { fprintf(stderr, "zkp_init: %s\n", zkp_strerror(rc)); return 2; }
    static const uint64_t g[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL,
                                   0x17f1d3a73197d794ULL, 0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL,
                                   0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    static const char eth_dst[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
    /* rows 0..2: the validators; row 3: their total; a fifth product, [12] g1, to compare with */
    const uint64_t sk[5][4] = {{3, 0, 0, 0}, {5, 0, 0, 0}, {9, 0, 0, 0}, {17, 0, 0, 0}, {12, 0, 0, 0}};
    uint64_t table[5 * 12];
    uint8_t tinf[5];
    rc = zkp_g1_mul_batch(ctx, g, 0, &sk[0][0], 5, table, tinf);
    if (rc != ZKP_OK) { fprintf(stderr, "keys: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 3; }
    const uint32_t idx[5] = {0, 2, 3, 1u | 0x80000000u, 0};
    const uint64_t seg_off[4] = {0, 2, 4, 4};
    uint64_t sum[3 * 12];
    uint8_t sinf[3], st[3];
    rc = zkp_g1_segment_sum_batch(ctx, table, 4, idx, 4, seg_off, 3, sum, sinf, st);
    if (rc != ZKP_OK) { fprintf(stderr, "segment sums: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 4; }
    if (memcmp(sum, table + 48, 96) || memcmp(sum + 12, table + 48, 96) || sinf[0] || sinf[1] || !sinf[2] || st[0] || st[1] || st[2]) {
        fprintf(stderr, "{0, 2} and total - {1} are not both [12] g1, or the empty segment is not the identity\n");
        return 5;
    }
    const uint8_t msg[3] = {'a', 'b', 'c'};
    const uint64_t offsets[2] = {0, 3};
    uint64_t hm[24], sig[24];
    uint8_t inf = 9, sig_inf = 9;
    rc = zkp_hash_to_g2_batch(ctx, msg, offsets, 1, (const uint8_t*)eth_dst, strlen(eth_dst), hm, &inf);
    if (rc == ZKP_OK) rc = zkp_g2_mul_batch(ctx, hm, 24, sk[4], 1, sig, &sig_inf);
    if (rc != ZKP_OK || inf || sig_inf) { fprintf(stderr, "sign: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 6; }
    const uint64_t rnd[2] = {0x9e3779b97f4a7c15ULL, 0xbf58476d1ce4e5b9ULL};
    const uint64_t one_seg[2] = {0, 2}, empty_seg[2] = {0, 0}, short_seg[2] = {0, 1};
    const uint32_t other[2] = {0, 1};
    int ok = -1;
    rc = zkp_bls_fast_aggregate_verify_batch(ctx, table, 4, idx, 2, one_seg, msg, offsets, (const uint8_t*)eth_dst, strlen(eth_dst), sig, NULL, 1, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 1) { fprintf(stderr, "verify: rc %d ok %d (%s)\n", rc, ok, zkp_last_error(ctx)); return 7; }
    rc = zkp_bls_fast_aggregate_verify_batch(ctx, table, 4, other, 2, one_seg, msg, offsets, (const uint8_t*)eth_dst, strlen(eth_dst), sig, NULL, 1, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "an aggregate verified under another committee: rc %d ok %d\n", rc, ok); return 8; }
    rc = zkp_bls_fast_aggregate_verify_batch(ctx, table, 4, idx, 0, empty_seg, msg, offsets, (const uint8_t*)eth_dst, strlen(eth_dst), sig, NULL, 1, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "an empty committee verified: rc %d ok %d\n", rc, ok); return 9; }
    if (zkp_g1_segment_sum_batch(ctx, table, 4, idx, 2, short_seg, 1, sum, sinf, st) != ZKP_ERR_ARG) {
        fprintf(stderr, "offsets that stop before the last entry were accepted\n");
        return 10;
    }
    printf("zkp_bls_agg ok: two committees sum to [12] g1, their aggregate signature verified, another committee and an empty one refused\n");
    zkp_free(ctx);
    return 0;
}
