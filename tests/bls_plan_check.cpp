// The planning header of hash-to-G2 and the BLS verifier (zkp_bls_plan.hpp) walked at the limits of the C ABI; built with
// g++ -fsanitize=address,undefined and run as a child process by tests/test_h2c_cpu.py.
#include <cassert>
#include <cstdio>
#include "zkp_bls_plan.hpp"
using namespace zkp::bls;
int main() {
    static_assert(sha_blocks(55) == 1 && sha_blocks(56) == 2 && sha_blocks(119) == 2 && sha_blocks(120) == 3, "padding boundary");
    for (size_t dst = 1; dst <= MAX_DST; dst++) {
        assert(bi_bytes(dst) == 34 + dst);
        assert(bi_blocks(dst) == (dst < 22 ? 1u : dst < 86 ? 2u : dst < 150 ? 3u : dst < 214 ? 4u : 5u));
        assert(tail_words(dst) * 4 + 32 == 64 * bi_blocks(dst) && tail_words(dst) <= TAIL_WORDS_MAX);
        for (size_t len = 0; len < 300; len++) {
            const size_t b = b0_bytes(len, dst), k = b0_blocks(len, dst);
            assert(b == 68 + len + dst && 64 * k >= b + 9 && 64 * (k - 1) < b + 9);
        }
    }
    assert(b0_bytes(8, 43) == 119 && b0_blocks(8, 43) == 2 && b0_blocks(9, 43) == 3 && b0_blocks(72, 43) == 3 && b0_blocks(73, 43) == 4);
    const size_t big = (size_t)1 << 40;
    assert(b0_blocks(big, 255) == (big + 68 + 255 + 9 + 63) / 64);
    assert(dst_bad(0) && dst_bad(256) && !dst_bad(1) && !dst_bad(255));
    const size_t ns[] = {1, 2, SLICE - 1, SLICE, SLICE + 1, MAX_VERIFY_N};
    for (size_t n : ns)
        for (int verify = 0; verify < 2; verify++) {
            const Layout L = layout(n, verify != 0);
            assert(L.slice == (n < SLICE ? n : SLICE));
            const size_t o[] = {L.tail0, L.tail, L.flag, L.neg_g1, L.neg_g1_inf, L.u, L.pts, L.hq, L.hinf, L.st, L.total};
            for (int i = 0; i + 1 < 11; i++) assert(o[i] % 256 == 0 && o[i] <= o[i + 1]);
            assert(L.tail - L.tail0 >= TAIL0_BYTES && L.flag - L.tail >= 4 * TAIL_WORDS_MAX && L.pts - L.u >= 192 * L.slice);
            assert(L.hq - L.pts >= 2 * L.slice * POINT_I32 * 4);
            if (verify) assert(L.hinf - L.hq >= 192 * n && L.st - L.hinf >= n && L.total - L.st >= 2 * n);
        }
    std::puts("ok");
    return 0;
}
