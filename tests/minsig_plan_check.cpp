// The planning header of hash-to-G1 and the min-sig BLS verifiers (zkp_bls_minsig_plan.hpp) walked at the limits of the C ABI; built with
// g++ -fsanitize=address,undefined and run as a child process by tests/test_h2g1_cpu.py.
#include <cassert>
#include <cstdio>
#include "zkp_bls_minsig_plan.hpp"
using namespace zkp::minsig;
int main() {
    static_assert(XMD_BYTES == 128 && XMD_BLOCKS == 4 && ISO_ROWS == 55 && POINT_I32 == 42 && H_EFF == 0xd201000000010001ull, "the suite");
    const size_t ns[] = {1, 2, SLICE - 1, SLICE, SLICE + 1, zkp::bls::MAX_VERIFY_N, zkp::bls::MAX_N};
    const Mode modes[] = {HASH, VERIFY, SAMEKEY};
    for (size_t n : ns)
        for (Mode mode : modes) {
            if (mode != HASH && n > zkp::bls::MAX_VERIFY_N) continue;
            const Layout L = layout(n, mode);
            assert(L.slice == (n < SLICE ? n : SLICE));
            const size_t o[] = {L.tail0, L.tail, L.flag, L.fixed_g2, L.fixed_inf2, L.u, L.pts, L.sums, L.hp, L.hinf, L.st, L.total};
            for (int i = 0; i + 1 < 12; i++) assert(o[i] % 256 == 0 && o[i] <= o[i + 1]);
            assert(L.tail - L.tail0 >= zkp::bls::TAIL0_BYTES && L.flag - L.tail >= 4 * zkp::bls::TAIL_WORDS_MAX && L.fixed_g2 - L.flag >= 4);
            assert(L.fixed_inf2 - L.fixed_g2 >= 2 * 192 && L.u - L.fixed_inf2 >= 2 && L.pts - L.u >= 96 * L.slice);
            assert(L.sums - L.pts >= 2 * L.slice * POINT_I32 * 4 && L.hp - L.sums >= L.slice * POINT_I32 * 4);
            const size_t per = mode == SAMEKEY ? 2 : 1;
            if (mode != HASH) assert(L.hinf - L.hp >= 96 * per * n && L.st - L.hinf >= per * n && L.total - L.st >= 2 * n + 1);
            // the last row the strided affine step writes: row (n - 1) * per of the hashed points, and for SAMEKEY row 2 n - 1 of the signatures
            if (mode != HASH) assert(12 * 8 * ((n - 1) * per + per) <= L.hinf - L.hp);
        }
    std::puts("ok");
    return 0;
}
