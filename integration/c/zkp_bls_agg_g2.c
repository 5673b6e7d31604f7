/* Pure-C consumer of include/zkp_bls_agg_g2.h: no Python, no torch.  Build:
 *   gcc -O2 -I include integration/c/zkp_bls_agg_g2.c -L zkvm_pairings_amd -lzkp_pairings -Wl,-rpath,$PWD/zkvm_pairings_amd -o zkp_bls_agg_g2
 * Two signers with the secret keys 3 and 5 sign "abc" and "abd" (min-pk: keys in G1, signatures in G2).  The G2 segment sum of the two
 * signatures is the aggregate, and "both minus the second" is the first signature again; AggregateVerify accepts the aggregate over the
 * two (key, message) pairs and refuses it with the keys swapped; a segment without a pair does not verify; offsets that do not end at the
 * number of messages are refused.  Then the min-sig layout: the keys [3] g2 and [5] g2 form a committee whose sum is [8] g2, and the
 * signature [8] H("abc") in G1 verifies under it. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zkp_bls_agg_g2.h"
#include "zkp_bls_minsig.h"

int main(void) {
    zkp_ctx* ctx = NULL;
    int rc = zkp_init(0, &ctx);
    if (rc != ZKP_OK) { fprintf(stderr, "zkp_init: %s\n", zkp_strerror(rc)); return 2; }
    static const uint64_t g1[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL,
                                    0x17f1d3a73197d794ULL, 0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL,
                                    0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    static const uint64_t g2[24] = {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL,
                                    0x024aa2b2f08f0a91ULL, 0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL,
                                    0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL, 0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL,
                                    0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL, 0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL,
                                    0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
    static const char eth_dst[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
    static const char net_dst[] = "BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_";
    const uint64_t sk[3][4] = {{3, 0, 0, 0}, {5, 0, 0, 0}, {8, 0, 0, 0}};
    uint64_t pk[2 * 12], hm[2 * 24], sig[2 * 24];
    uint8_t inf[2] = {9, 9}, hinf[2] = {9, 9}, sinf[2] = {9, 9};
    const uint8_t msgs[6] = {'a', 'b', 'c', 'a', 'b', 'd'};
    const uint64_t offsets[3] = {0, 3, 6};
    rc = zkp_g1_mul_batch(ctx, g1, 0, &sk[0][0], 2, pk, inf);
    if (rc == ZKP_OK) rc = zkp_hash_to_g2_batch(ctx, msgs, offsets, 2, (const uint8_t*)eth_dst, strlen(eth_dst), hm, hinf);
    if (rc == ZKP_OK) rc = zkp_g2_mul_batch(ctx, hm, 24, &sk[0][0], 2, sig, sinf);
    if (rc != ZKP_OK || inf[0] || inf[1] || hinf[0] || hinf[1] || sinf[0] || sinf[1]) {
        fprintf(stderr, "keys and signatures: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx));
        return 3;
    }
    /* segment 0: both signatures; segment 1: both and the second subtracted; segment 2: empty */
    const uint32_t idx[5] = {0, 1, 0, 1, 1u | 0x80000000u};
    const uint64_t seg_off[4] = {0, 2, 5, 5};
    uint64_t sum[3 * 24];
    uint8_t oinf[3], st[3];
    rc = zkp_g2_segment_sum_batch(ctx, sig, 2, idx, 5, seg_off, 3, sum, oinf, st);
    if (rc != ZKP_OK) { fprintf(stderr, "segment sums: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 4; }
    if (memcmp(sum + 24, sig, 192) || !memcmp(sum, sig, 192) || oinf[0] || oinf[1] || !oinf[2] || st[0] || st[1] || st[2]) {
        fprintf(stderr, "both minus the second is not the first signature, or the empty segment is not the identity\n");
        return 5;
    }
    const uint64_t rnd[2] = {0x9e3779b97f4a7c15ULL, 0xbf58476d1ce4e5b9ULL};
    const uint64_t one_sig[2] = {0, 2}, short_seg[2] = {0, 1}, with_empty[3] = {0, 2, 2};
    uint64_t swapped[2 * 12], two_sig[2 * 24];
    const uint64_t rnd2[4] = {0x9e3779b97f4a7c15ULL, 0xbf58476d1ce4e5b9ULL, 0x94d049bb133111ebULL, 0x2545f4914f6cdd1dULL};
    memcpy(swapped, pk + 12, 96);
    memcpy(swapped + 12, pk, 96);
    memcpy(two_sig, sum, 192);
    memcpy(two_sig + 24, sum, 192);
    int ok = -1;
    rc = zkp_bls_aggregate_verify_batch(ctx, pk, NULL, msgs, offsets, 2, one_sig, (const uint8_t*)eth_dst, strlen(eth_dst), sum, NULL, 1, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 1) { fprintf(stderr, "AggregateVerify: rc %d ok %d (%s)\n", rc, ok, zkp_last_error(ctx)); return 6; }
    rc = zkp_bls_aggregate_verify_batch(ctx, swapped, NULL, msgs, offsets, 2, one_sig, (const uint8_t*)eth_dst, strlen(eth_dst), sum, NULL, 1, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "an aggregate verified with its keys swapped: rc %d ok %d\n", rc, ok); return 7; }
    rc = zkp_bls_aggregate_verify_batch(ctx, pk, NULL, msgs, offsets, 2, with_empty, (const uint8_t*)eth_dst, strlen(eth_dst), two_sig, NULL, 2, rnd2, 0, &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "a signature over no pair verified: rc %d ok %d\n", rc, ok); return 8; }
    if (zkp_bls_aggregate_verify_batch(ctx, pk, NULL, msgs, offsets, 2, short_seg, (const uint8_t*)eth_dst, strlen(eth_dst), sum, NULL, 1, rnd, 0, &ok) !=
        ZKP_ERR_ARG) {
        fprintf(stderr, "offsets that stop before the last message were accepted\n");
        return 9;
    }
    /* the min-sig layout: a committee of two G2 keys */
    uint64_t table[2 * 24], h1[12], agg[12];
    uint8_t tinf[2] = {9, 9}, h1inf = 9, ainf = 9;
    const uint32_t members[2] = {0, 1};
    rc = zkp_g2_mul_batch(ctx, g2, 0, &sk[0][0], 2, table, tinf);
    if (rc == ZKP_OK) rc = zkp_hash_to_g1_batch(ctx, msgs, offsets, 1, (const uint8_t*)net_dst, strlen(net_dst), h1, &h1inf);
    if (rc == ZKP_OK) rc = zkp_g1_mul_batch(ctx, h1, 12, sk[2], 1, agg, &ainf);
    if (rc != ZKP_OK || tinf[0] || tinf[1] || h1inf || ainf) { fprintf(stderr, "min-sig keys: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 10; }
    rc = zkp_bls_minsig_fast_aggregate_verify_batch(ctx, table, 2, members, 2, one_sig, msgs, offsets, (const uint8_t*)net_dst, strlen(net_dst), agg, NULL, 1,
                                                    rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 1) { fprintf(stderr, "min-sig committee: rc %d ok %d (%s)\n", rc, ok, zkp_last_error(ctx)); return 11; }
    rc = zkp_bls_minsig_fast_aggregate_verify_batch(ctx, table, 2, members, 1, short_seg, msgs, offsets, (const uint8_t*)net_dst, strlen(net_dst), agg, NULL, 1,
                                                    rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "the aggregate verified under half its committee: rc %d ok %d\n", rc, ok); return 12; }
    printf("zkp_bls_agg_g2 ok: two signatures aggregated and verified over two pairs, swapped keys and an empty segment refused, a G2 committee verified\n");
    zkp_free(ctx);
    return 0;
}
