/* Pure-C consumer of include/zkp_bls_minsig.h: no Python, no torch.  Build:
 *   gcc -O2 -I include integration/c/zkp_bls_minsig.c -L zkvm_pairings_amd -lzkp_pairings -Wl,-rpath,$PWD/zkvm_pairings_amd -o zkp_bls_minsig
 * "abc" hashed to G1 under the tag of RFC 9380 appendix J.9.1 must be that appendix's point.  Then a beacon with the secret key 5: its
 * public key [5] g2, its signatures [5] H(m) in G1 under drand's quicknet tag on two rounds, verified by the general verifier and by the
 * same-key verifier, both refusing a changed message, and the refusal of an empty tag. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zkp_bls_minsig.h"

int main(void) {
    zkp_ctx* ctx = NULL;
    int rc = zkp_init(0, &ctx);
    if (rc != ZKP_OK) { fprintf(stderr, "zkp_init: %s\n", zkp_strerror(rc)); return 2; }
    static const uint64_t g2[24] = {
        0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL,
        0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL, 0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL,
        0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL,
        0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL,
        0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL, 0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL,
        0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
    static const uint64_t want[12] = {
        0xd3c68900be2f6903ULL, 0xee664ba5379a7655ULL, 0xa9a7943388a49a3aULL, 0x139cc0b2f284dca0ULL,
        0x2ab2ecdf6a96ef1cULL, 0x03567bc5ef9c690cULL, 0xb88176c229f2885dULL, 0x1f0b8dfaaa154fa6ULL,
        0xc85b67af21553331ULL, 0x8f3b28be689c8429ULL, 0x211f346271d7b01cULL, 0x0b9c15f3fe6e5cf4ULL};
    static const char rfc_dst[] = "QUUX-V01-CS02-with-BLS12381G1_XMD:SHA-256_SSWU_RO_";
    static const char net_dst[] = "BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_";
    const uint8_t abc[3] = {'a', 'b', 'c'};
    const uint64_t one[2] = {0, 3};
    uint64_t hm[24], sig[24], pk[48];
    uint8_t inf[2] = {9, 9}, sig_inf[2] = {9, 9}, pk_inf[2] = {9, 9};
    rc = zkp_hash_to_g1_batch(ctx, abc, one, 1, (const uint8_t*)rfc_dst, strlen(rfc_dst), hm, inf);
    if (rc != ZKP_OK || inf[0]) { fprintf(stderr, "hash: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 3; }
    if (memcmp(hm, want, sizeof want)) { fprintf(stderr, "hash_to_g1(\"abc\") is not the point of RFC 9380 J.9.1\n"); return 4; }
    const uint8_t rounds[5] = {'r', '1', 'r', '2', '!'};
    const uint64_t offsets[3] = {0, 2, 5};
    const uint64_t sk[8] = {5, 0, 0, 0, 5, 0, 0, 0};
    rc = zkp_hash_to_g1_batch(ctx, rounds, offsets, 2, (const uint8_t*)net_dst, strlen(net_dst), hm, inf);
    if (rc == ZKP_OK) rc = zkp_g1_mul_batch(ctx, hm, 12, sk, 2, sig, sig_inf);
    if (rc == ZKP_OK) rc = zkp_g2_mul_batch(ctx, g2, 0, sk, 2, pk, pk_inf);
    if (rc != ZKP_OK || inf[0] || inf[1] || sig_inf[0] || sig_inf[1] || pk_inf[0] || pk_inf[1]) {
        fprintf(stderr, "sign: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx));
        return 5;
    }
    const uint64_t rnd[4] = {0x9e3779b97f4a7c15ULL, 0xbf58476d1ce4e5b9ULL, 0x94d049bb133111ebULL, 0x2545f4914f6cdd1dULL};
    int ok = -1;
    rc = zkp_bls_minsig_verify_batch(ctx, pk, NULL, rounds, offsets, (const uint8_t*)net_dst, strlen(net_dst), sig, NULL, 2, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 1) { fprintf(stderr, "verify: rc %d ok %d (%s)\n", rc, ok, zkp_last_error(ctx)); return 6; }
    rc = zkp_bls_minsig_verify_samekey_batch(ctx, pk, rounds, offsets, (const uint8_t*)net_dst, strlen(net_dst), sig, NULL, 2, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 1) { fprintf(stderr, "same-key verify: rc %d ok %d (%s)\n", rc, ok, zkp_last_error(ctx)); return 7; }
    const uint8_t other[5] = {'r', '1', 'r', '3', '!'};
    rc = zkp_bls_minsig_verify_batch(ctx, pk, NULL, other, offsets, (const uint8_t*)net_dst, strlen(net_dst), sig, NULL, 2, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "a signature verified on another message: rc %d ok %d\n", rc, ok); return 8; }
    rc = zkp_bls_minsig_verify_samekey_batch(ctx, pk, other, offsets, (const uint8_t*)net_dst, strlen(net_dst), sig, NULL, 2, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "the same-key verifier accepted another message: rc %d ok %d\n", rc, ok); return 9; }
    if (zkp_hash_to_g1_batch(ctx, abc, one, 1, (const uint8_t*)net_dst, 0, hm, inf) != ZKP_ERR_ARG) {
        fprintf(stderr, "an empty tag was accepted\n");
        return 10;
    }
    printf("zkp_bls_minsig ok: the RFC 9380 point of \"abc\", two beacon rounds verified by both verifiers, a changed round refused by both\n");
    zkp_free(ctx);
    return 0;
}
