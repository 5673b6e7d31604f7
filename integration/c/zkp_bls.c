/* Pure-C consumer of include/zkp_bls.h: no Python, no torch.  Build:
 *   gcc -O2 -I include integration/c/zkp_bls.c -L zkvm_pairings_amd -lzkp_pairings -Wl,-rpath,$PWD/zkvm_pairings_amd -o zkp_bls
 * "abc" hashed to G2 under the tag of RFC 9380 appendix J.10.1 must be that appendix's point.  Then a validator with the secret key 5:
 * its public key [5] g1, its signature [5] H(m) under Ethereum's tag, one verification that holds, one on a changed message that does
 * not, and the refusal of an empty tag. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zkp_bls.h"

int main(void) {
    zkp_ctx* ctx = NULL;
    int rc = zkp_init(0, &ctx);
    if (rc != ZKP_OK) { fprintf(stderr, "zkp_init: %s\n", zkp_strerror(rc)); return 2; }
    static const uint64_t g[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL,
                                   0x17f1d3a73197d794ULL, 0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL,
                                   0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    static const uint64_t want[24] = {
        0x4168aff2787776e6ULL, 0xc7780ccc7954725fULL, 0x0e7a210245129dbeULL, 0x00d80ccd5ba4b7feULL,
        0x62aae3cab37a27ceULL, 0x02c2d18e033b9605ULL, 0xa2acf73a41177fd8ULL, 0xca3a230ed250fbe3ULL,
        0x374de9eb4b41dfe4ULL, 0x6f83f175e80b06fcULL, 0x9623efd38c49f81aULL, 0x139cddbccdc5e91bULL,
        0xfb87bf7466b2ba48ULL, 0xeb197642555a0645ULL, 0xbe6ea05c4cfe244aULL, 0x4bcb1e621d3a7202ULL,
        0xa37440985269cf58ULL, 0x1787327b68159716ULL, 0xf106d4cec0eddd16ULL, 0x1ce70dd94a733534ULL,
        0x03866e9f3d49ac1eULL, 0xf3001578f71c694eULL, 0xd10ecd2c50f8a1baULL, 0x00aa65dae3c8d732ULL};
    static const char rfc_dst[] = "QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_RO_";
    static const char eth_dst[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
    const uint8_t msg[3] = {'a', 'b', 'c'};
    const uint64_t offsets[2] = {0, 3};
    uint64_t hm[24], sig[24], pk[12];
    uint8_t inf = 9, sig_inf = 9, pk_inf = 9;
    rc = zkp_hash_to_g2_batch(ctx, msg, offsets, 1, (const uint8_t*)rfc_dst, strlen(rfc_dst), hm, &inf);
    if (rc != ZKP_OK || inf) { fprintf(stderr, "hash: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 3; }
    if (memcmp(hm, want, sizeof want)) { fprintf(stderr, "hash_to_g2(\"abc\") is not the point of RFC 9380 J.10.1\n"); return 4; }
    const uint64_t sk[4] = {5, 0, 0, 0};
    rc = zkp_hash_to_g2_batch(ctx, msg, offsets, 1, (const uint8_t*)eth_dst, strlen(eth_dst), hm, &inf);
    if (rc == ZKP_OK) rc = zkp_g2_mul_batch(ctx, hm, 24, sk, 1, sig, &sig_inf);
    if (rc == ZKP_OK) rc = zkp_g1_mul_batch(ctx, g, 12, sk, 1, pk, &pk_inf);
    if (rc != ZKP_OK || inf || sig_inf || pk_inf) { fprintf(stderr, "sign: %s (%s)\n", zkp_strerror(rc), zkp_last_error(ctx)); return 5; }
    const uint64_t rnd[2] = {0x9e3779b97f4a7c15ULL, 0xbf58476d1ce4e5b9ULL};
    int ok = -1;
    rc = zkp_bls_verify_batch(ctx, pk, NULL, msg, offsets, (const uint8_t*)eth_dst, strlen(eth_dst), sig, NULL, 1, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 1) { fprintf(stderr, "verify: rc %d ok %d (%s)\n", rc, ok, zkp_last_error(ctx)); return 6; }
    const uint8_t other[3] = {'a', 'b', 'd'};
    rc = zkp_bls_verify_batch(ctx, pk, NULL, other, offsets, (const uint8_t*)eth_dst, strlen(eth_dst), sig, NULL, 1, rnd, 0, &ok);
    if (rc != ZKP_OK || ok != 0) { fprintf(stderr, "a signature verified on another message: rc %d ok %d\n", rc, ok); return 7; }
    if (zkp_hash_to_g2_batch(ctx, msg, offsets, 1, (const uint8_t*)eth_dst, 0, hm, &inf) != ZKP_ERR_ARG) {
        fprintf(stderr, "an empty tag was accepted\n");
        return 8;
    }
    printf("zkp_bls ok: the RFC 9380 point of \"abc\", a signature verified, the same signature refused on another message\n");
    zkp_free(ctx);
    return 0;
}
