// zkp_h2f.hpp -- what the two hash_to_field kernels share (zkp_bls.hip: Fp2, eight blocks of expand_message_xmd; zkp_bls_minsig.hip: Fp, four
// blocks): SHA-256 with its rolling schedule, the words b_0 absorbs, the wide reduction on the 28-bit core, and the bodies of the tails
// kernel and of the lane-per-message kernel with the number of output blocks as a template argument.  Plain C++ over zkp_fp28.hpp: the
// host builds of tests/bls_kernel_host.cpp and tests/minsig_kernel_host.cpp take it as it is.
#pragma once
#include "zkp_bls_plan.hpp"
#include "zkp_fp28.hpp"

namespace zkp {
namespace h2f {

using zkp28::Fp28;
using zkp28::NL;

// ------------------------------------------------------------------------------------------- SHA-256
__device__ __constant__ const uint32_t K_SHA[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ __forceinline__ uint32_t rotr(uint32_t x, int r) { return __builtin_rotateright32(x, r); }
__device__ __forceinline__ void sha_init(uint32_t* h) {
    h[0] = 0x6a09e667; h[1] = 0xbb67ae85; h[2] = 0x3c6ef372; h[3] = 0xa54ff53a;
    h[4] = 0x510e527f; h[5] = 0x9b05688c; h[6] = 0x1f83d9ab; h[7] = 0x5be0cd19;
}
// one block: h += compress(h, w); w (16 words, big-endian order) is the rolling schedule and is destroyed
__device__ __forceinline__ void sha_block(uint32_t* h, uint32_t* w) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
            const uint32_t s0 = rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3), s1 = rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10);
            w[t & 15] += s0 + w[(t + 9) & 15] + s1;
        }
        const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K_SHA[t] + w[t & 15];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// word `pos / 4` of the stream b_0 absorbs after Z_pad: msg | tail0 | 0x80 | zeros | the bit length in the last eight bytes of `padded`
__device__ __forceinline__ uint32_t b0_word(const uint8_t* msg, uint64_t len, const uint8_t* tail0, uint64_t total, uint64_t padded, uint64_t bits,
                                            uint64_t pos) {
    if (pos + 4 <= len) {
        const uint8_t* p = msg + pos;
        if (((uintptr_t)p & 3) == 0) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(p));
        return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint64_t q = pos + k;
        uint32_t byte = 0;
        if (q < len) byte = msg[q];
        else if (q < total) byte = tail0[q - len];
        else if (q == total) byte = 0x80;
        else if (q >= padded - 8) byte = (uint32_t)(bits >> (8 * (padded - 1 - q))) & 0xff;
        v = (v << 8) | byte;
    }
    return v;
}

// 256 bits as eight big-endian words (be[0] the most significant) -> 14 unsigned 28-bit limbs
__device__ __forceinline__ void limbs_from_be256(int32_t* l, const uint32_t* be) {
    uint32_t v[9];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = be[7 - k];
    v[8] = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const int bit = 28 * i, word = bit >> 5, sh = bit & 31;
        if (word >= 8) {
            l[i] = 0;
        } else {
            const uint64_t t = (uint64_t)v[word] | ((uint64_t)v[word + 1] << 32);
            l[i] = (int32_t)((t >> sh) & (uint64_t)zkp28::MASK);
        }
    }
}
// OS2IP(hi | lo) mod p, canonical: (lo R^2 + hi 2^256 R^2) / R in one reduction (limbs below 2^28 against balanced constants: La Lb = 2 each)
__device__ __forceinline__ void reduce_wide(uint64_t* out, const uint32_t* hi, const uint32_t* lo) {
    Fp28 h, l, r2, w, r;
    limbs_from_be256(h.l, hi);
    limbs_from_be256(l.l, lo);
#pragma unroll
    for (int i = 0; i < NL; i++) {
        r2.l[i] = zkp28::K28_R2[i];
        w.l[i] = zkp28::K28_W256R[i];
    }
    zkp28::mont_mul_ps<true>(r.l, l.l, r2.l, h.l, w.l);
    zkp28::fp28_to_wire(out, r);
}

// the two tails every message shares, for an expansion to `xmd_bytes` bytes (I2OSP(xmd_bytes, 2) opens tail0)
__device__ __forceinline__ void tails_body(const uint8_t* dst, uint32_t dst_len, uint32_t xmd_bytes, uint8_t* tail0, uint32_t* tail) {
    tail0[0] = (uint8_t)(xmd_bytes >> 8);   // I2OSP(xmd_bytes, 2)
    tail0[1] = (uint8_t)xmd_bytes;
    tail0[2] = 0;                       // I2OSP(0, 1)
    for (uint32_t i = 0; i < dst_len; i++) tail0[3 + i] = dst[i];
    tail0[3 + dst_len] = (uint8_t)dst_len;
    const uint32_t bytes = (uint32_t)bls::tail_words(dst_len) * 4, bits = 8 * (uint32_t)bls::bi_bytes(dst_len);
    for (uint32_t wd = 0; wd < bytes / 4; wd++) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t q = 4 * wd + k;   // the stream position is 32 + q; q = 0 is the block counter's byte
            uint32_t byte = 0;
            if (q >= 1 && q <= dst_len) byte = dst[q - 1];
            else if (q == dst_len + 1) byte = dst_len;
            else if (q == dst_len + 2) byte = 0x80;
            else if (q >= bytes - 4) byte = (bits >> (8 * (bytes - 1 - q))) & 0xff;
            v = (v << 8) | byte;
        }
        tail[wd] = v;
    }
}

// lane i < n of a launch on messages at .. at + n - 1 of n_all: expand_message_xmd to 32 NBLK bytes, each 64-byte slice reduced mod p;
// out: n x NBLK / 2 field elements of 6 words.  A message whose offsets decrease or leave [offsets[0], offsets[n_all]] is hashed as the
// empty one - nothing outside that range is ever read - and raises *bad (the validation word; null outside validation mode).
template <uint32_t NBLK>
__device__ __forceinline__ void h2f_body(const uint8_t* msgs, const uint64_t* offsets, uint64_t at, uint32_t i, uint64_t n_all, const uint8_t* tail0,
                                         const uint32_t* tail, uint32_t dst_len, uint64_t* out, int* bad) {
    const uint64_t first = offsets[0], last = offsets[n_all], lo = offsets[at + i], hi = offsets[at + i + 1];
    const bool sound = first <= lo && lo <= hi && hi <= last;
    const uint64_t len = sound ? hi - lo : 0;
    if (!sound && bad) atomicOr(bad, 1);
    const uint8_t* msg = msgs + lo;
    const uint64_t total = len + 4 + dst_len;                      // bytes after Z_pad
    const uint64_t blocks = (64 + total + 9 + 63) / 64 - 1;        // ... and their blocks, the padding included
    const uint64_t padded = 64 * blocks, bits = 8 * (64 + total);
    uint32_t b0[8], w[16];
    sha_init(b0);
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = 0;
    sha_block(b0, w);                                              // Z_pad
#pragma unroll 1
    for (uint64_t blk = 0; blk < blocks; blk++) {
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = b0_word(msg, len, tail0, total, padded, bits, 64 * blk + 4 * k);
        sha_block(b0, w);
    }
    const uint32_t nbi = (uint32_t)bls::bi_blocks(dst_len);
    uint32_t prev[8], keep[8], h[8];
#pragma unroll
    for (int k = 0; k < 8; k++) prev[k] = 0;
#pragma unroll 1
    for (uint32_t j = 1; j <= NBLK; j++) {
        sha_init(h);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            w[k] = b0[k] ^ prev[k];                                // b_0 alone for j = 1
            w[8 + k] = tail[k];
        }
        w[8] |= j << 24;
        sha_block(h, w);
#pragma unroll 1
        for (uint32_t blk = 1; blk < nbi; blk++) {
#pragma unroll
            for (int k = 0; k < 16; k++) w[k] = tail[8 + 16 * (blk - 1) + k];
            sha_block(h, w);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) prev[k] = h[k];
        if (j & 1) {
#pragma unroll
            for (int k = 0; k < 8; k++) keep[k] = h[k];
        } else {
            uint64_t o[6];
            reduce_wide(o, keep, h);
#pragma unroll
            for (int k = 0; k < 6; k++) out[(size_t)i * (3 * NBLK) + (j / 2 - 1) * 6 + k] = o[k];
        }
    }
}

}  // namespace h2f
}  // namespace zkp
