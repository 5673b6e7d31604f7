// zkp_bls_plan.hpp -- sizes of the hash-to-G2 pipeline and of the BLS batch verifier (zkp_bls.hip): SHA-256 block counts per message and
// per DST length, the slice of messages one pass maps, the workspace layout, the limits of the C ABI.  Plain C++: a host compiler takes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkp {
namespace bls {

constexpr size_t MAX_DST = 255;                       // RFC 9380 5.3.1; longer tags (5.3.3) are out of scope
constexpr size_t MAX_N = ((size_t)1 << 31) - 1;       // messages / points of one hash or map call: every launch count stays in 32 bits
constexpr size_t MAX_VERIFY_N = (size_t)1 << 24;      // the RLC driver's limit with a column (zkp_rlc_plan.hpp)
constexpr size_t L_BYTES = 64;                        // ceil((381 + 128) / 8) bytes per field element
constexpr size_t XMD_BYTES = 4 * L_BYTES;             // count = 2, m = 2
constexpr size_t XMD_BLOCKS = XMD_BYTES / 32;         // b_1 .. b_8
constexpr size_t SLICE = (size_t)1 << 17;             // messages mapped per pass: bounds the workspace of projective points
constexpr size_t POINT_I32 = 6 * 14;                  // a projective point of E2: three Fp2 of 14 limbs
constexpr size_t TAIL0_BYTES = 4 + MAX_DST;           // I2OSP(256, 2) | 0 | DST | len(DST): what b_0 absorbs after the message

// SHA-256 blocks that absorb `bytes` bytes: the 0x80 byte and the 64-bit length need nine more
constexpr size_t sha_blocks(size_t bytes) { return (bytes + 9 + 63) / 64; }
// b_0 = H(Z_pad | msg | I2OSP(256, 2) | 0 | DST | len(DST))
constexpr size_t b0_bytes(size_t msg_len, size_t dst_len) { return 64 + msg_len + 3 + dst_len + 1; }
constexpr size_t b0_blocks(size_t msg_len, size_t dst_len) { return sha_blocks(b0_bytes(msg_len, dst_len)); }
// b_i = H((b_0 ^ b_(i-1)) | i | DST | len(DST))
constexpr size_t bi_bytes(size_t dst_len) { return 32 + 1 + dst_len + 1; }
constexpr size_t bi_blocks(size_t dst_len) { return sha_blocks(bi_bytes(dst_len)); }
// the padded tail of every b_i after its first 32 bytes, as big-endian words: i's byte (left zero), DST, len(DST), 0x80, zeros, the bit length
constexpr size_t tail_words(size_t dst_len) { return (64 * bi_blocks(dst_len) - 32) / 4; }
constexpr size_t TAIL_WORDS_MAX = tail_words(MAX_DST);

constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline bool dst_bad(size_t dst_len) { return dst_len == 0 || dst_len > MAX_DST; }

// the workspace of a call on n messages / points: the two DST tails, the slice's u values and projective points, and for the verifier
// the hashed points, their infinity bytes, the status bytes of the points check, -g1 and the flag word
struct Layout {
    size_t tail0, tail, flag, neg_g1, neg_g1_inf, u, pts, hq, hinf, st, total;
    size_t slice;
};
inline Layout layout(size_t n, bool verify) {
    Layout L;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
    L.slice = n < SLICE ? n : SLICE;
    L.tail0 = take(TAIL0_BYTES);
    L.tail = take(TAIL_WORDS_MAX * 4);
    L.flag = take(4 * sizeof(int));
    L.neg_g1 = take(96);
    L.neg_g1_inf = take(1);
    L.u = take(L.slice * 192);
    L.pts = take(2 * L.slice * POINT_I32 * 4);
    L.hq = take(verify ? n * 192 : 0);
    L.hinf = take(verify ? n : 0);
    L.st = take(verify ? 2 * n : 0);
    L.total = at;
    return L;
}

}  // namespace bls
}  // namespace zkp
