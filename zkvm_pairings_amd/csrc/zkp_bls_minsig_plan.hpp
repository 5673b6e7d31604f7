// zkp_bls_minsig_plan.hpp -- sizes of the hash-to-G1 pipeline and of the minimal-signature-size BLS verifiers (zkp_bls_minsig.hip): the
// expansion's length, the slice of messages one pass maps, the workspace layout.  The SHA-256 block counts, the tails and the limits of
// the C ABI are zkp_bls_plan.hpp's.  Plain C++: a host compiler takes it.
#pragma once
#include "zkp_bls_plan.hpp"

namespace zkp {
namespace minsig {

constexpr size_t XMD_BYTES = 2 * bls::L_BYTES;        // count = 2, m = 1
constexpr size_t XMD_BLOCKS = XMD_BYTES / 32;         // b_1 .. b_4
constexpr size_t SLICE = bls::SLICE;                  // messages mapped per pass
constexpr size_t POINT_I32 = 3 * 14;                  // a projective point of E: three Fp of 14 limbs
constexpr size_t ISO_ROWS = 12 + 11 + 16 + 16;        // x_num, x_den, y_num, y_den of the 11-isogeny, from x^0 up
constexpr uint64_t H_EFF = 0xd201000000010001ull;     // 1 - x

enum Mode { HASH = 0, VERIFY = 1, SAMEKEY = 2 };

// the workspace of a call on n messages / points: the two DST tails, the slice's u values, mapped points and cleared sums, and for the
// verifiers the flag word, the fixed G2 points (-g2; for the same-key verifier the key before it) with their infinity bytes, the hashed
// points (SAMEKEY: the n x 2 rows of the driver's columns, H(m_i) beside sig_i), their infinity bytes and the status bytes
struct Layout {
    size_t tail0, tail, flag, fixed_g2, fixed_inf2, u, pts, sums, hp, hinf, st, total;
    size_t slice;
};
inline Layout layout(size_t n, Mode mode) {
    Layout L;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += bls::align256(bytes); return o; };
    const size_t per = mode == SAMEKEY ? 2 : 1;
    L.slice = n < SLICE ? n : SLICE;
    L.tail0 = take(bls::TAIL0_BYTES);
    L.tail = take(bls::TAIL_WORDS_MAX * 4);
    L.flag = take(4 * sizeof(int));
    L.fixed_g2 = take(2 * 192);
    L.fixed_inf2 = take(2);
    L.u = take(L.slice * 96);
    L.pts = take(2 * L.slice * POINT_I32 * 4);
    L.sums = take(L.slice * POINT_I32 * 4);
    L.hp = take(mode == HASH ? 0 : n * per * 96);
    L.hinf = take(mode == HASH ? 0 : n * per);
    L.st = take(mode == HASH ? 0 : 2 * n + 1);       // VERIFY: pk, sig; SAMEKEY: sig, the key
    L.total = at;
    return L;
}

}  // namespace minsig
}  // namespace zkp
