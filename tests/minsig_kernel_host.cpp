// minsig_kernel_host.cpp -- the kernels of zkvm_pairings_amd/csrc/zkp_bls_minsig.hip that keep to one lane (k_g1h_tails, k_g1h_field: the
// shared SHA-256 / expander / wide reduction of zkp_h2f.hpp with four blocks; k_g1h_map: the straight-line SSWU, its one exponentiation,
// the 11-isogeny on a fraction; k_g1h_clear: the complete additions and the 64-bit double-and-add) compiled for the HOST and run as
// written, in the manner of tests/bls_kernel_host.cpp: the lanes of a launch one after the other.  tests/test_h2g1_cpu.py builds this
// with g++ -fsanitize=address,undefined, runs it as a child process and compares what the kernels leave with tests/h2g1_model.py.
// Every buffer is allocated EXACTLY.  CPU only: nothing here touches HIP.  k_g1h_affine exchanges values between the lanes of a
// wavefront through LDS and is not here: the projective points are written out and the test divides.
//
//   minsig_kernel_host <in> <out>
//   in:  u64 dst_len | u64 n | u64 n_u | u64 n_pts | u64 base | dst | offsets (n + 1 u64, absolute: the first is base) | the bytes
//        [base, offsets[n]) | n_u x 2 field elements (48 B each, canonical) | n_pts wire points (96 B) | n_pts infinity bytes
//   out: u (n x 96 B) | n_u projective points (X, Y, Z: 3 x 48 B canonical) of k_g1h_map + k_g1h_clear | n_pts of k_g1h_clear on the
//        wire points | the validation word (4 B)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define ZKP_MINSIG_KERNELS_ONLY
#define ZKP_FP28_HOST
#define __global__
#define __device__
#define __constant__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __builtin_rotateright32(x, r) ((uint32_t)(((x) >> (r)) | ((x) << (32 - (r)))))
struct D3 { unsigned x; };
static D3 threadIdx, blockIdx;
static int atomicOr(int* p, int v) {
    const int old = *p;
    *p |= v;
    return old;
}
#include "../zkvm_pairings_amd/csrc/zkp_bls_minsig.hip"

using namespace zkp;
template <class F> static void launch(unsigned grid, unsigned block, F f) {
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = 0; t < block; t++) {
            blockIdx.x = b;
            threadIdx.x = t;
            f();
        }
}
// exactly `bytes` bytes (at least one is allocated, none of it readable beyond `bytes` under the sanitizer's red zones)
static uint8_t* exact(size_t bytes) { return (uint8_t*)malloc(bytes ? bytes : 1); }

// slot `slot` of a planar workspace as three canonical values
static void dump(FILE* o, const int32_t* ws, size_t stride, size_t slot) {
    for (int v = 0; v < 3; v++) {
        zkp28::Fp28 a;
        for (int k = 0; k < 14; k++) a.l[k] = ws[(size_t)(14 * v + k) * stride + slot];
        uint64_t w[6];
        zkp28::fp28_to_wire(w, a);
        fwrite(w, 8, 6, o);
    }
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hd[5];
    if (fread(hd, 8, 5, f) != 5) return 2;
    const uint64_t dst_len = hd[0], n = hd[1], n_u = hd[2], n_pts = hd[3], base = hd[4];
    if (bls::dst_bad(dst_len) || n > 4096 || n_u > 4096 || n_pts > 4096) return 2;
    uint8_t* dst = exact(dst_len);
    std::vector<uint64_t> offsets(n + 1);
    if (fread(dst, 1, dst_len, f) != dst_len || fread(offsets.data(), 8, n + 1, f) != n + 1) return 2;
    const uint64_t end = offsets[n] >= base ? offsets[n] : base;
    const size_t buf_len = (size_t)(end - base);
    uint8_t* buf = exact(buf_len);
    if (fread(buf, 1, buf_len, f) != buf_len) return 2;
    uint64_t* uin = (uint64_t*)exact(96 * n_u);
    uint64_t* pin = (uint64_t*)exact(96 * n_pts);
    uint8_t* pinf = exact(n_pts);
    if (fread(uin, 1, 96 * n_u, f) != 96 * n_u || fread(pin, 1, 96 * n_pts, f) != 96 * n_pts || fread(pinf, 1, n_pts, f) != n_pts) return 2;
    fclose(f);

    uint8_t* tail0 = exact(dst_len + 4);
    uint32_t* tail = (uint32_t*)exact(bls::tail_words(dst_len) * 4);
    uint64_t* u = (uint64_t*)exact(n * 96);
    int bad = 0;
    const uint8_t* msgs = (const uint8_t*)((uintptr_t)buf - (uintptr_t)base);
    launch(1, 1, [&] { k_g1h_tails(dst, (uint32_t)dst_len, tail0, tail); });
    if (n) launch((unsigned)((n + TPB_H - 1) / TPB_H), TPB_H, [&] { k_g1h_field(msgs, offsets.data(), 0, (uint32_t)n, n, tail0, tail, (uint32_t)dst_len, u, &bad); });

    // the map's workspace has 2 n_u slots, the sums n_u (n_pts): the strides are the slot counts, nothing to spare
    int32_t* mapped = (int32_t*)exact(2 * n_u * minsig::POINT_I32 * 4);
    int32_t* sums = (int32_t*)exact(n_u * minsig::POINT_I32 * 4);
    int32_t* cleared = (int32_t*)exact(n_pts * minsig::POINT_I32 * 4);
    if (n_u) {
        launch((unsigned)((2 * n_u + TPB_M - 1) / TPB_M), TPB_M, [&] { k_g1h_map(uin, (uint32_t)(2 * n_u), mapped, 2 * n_u); });
        launch((unsigned)((n_u + TPB_M - 1) / TPB_M), TPB_M, [&] { k_g1h_clear<false>(nullptr, nullptr, mapped, 2 * n_u, (uint32_t)n_u, sums, n_u); });
    }
    if (n_pts) launch((unsigned)((n_pts + TPB_M - 1) / TPB_M), TPB_M, [&] { k_g1h_clear<true>(pin, pinf, nullptr, 0, (uint32_t)n_pts, cleared, n_pts); });

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(u, 1, n * 96, o);
    for (size_t i = 0; i < n_u; i++) dump(o, sums, n_u, i);
    for (size_t i = 0; i < n_pts; i++) dump(o, cleared, n_pts, i);
    const int32_t word = bad;
    fwrite(&word, 4, 1, o);
    fclose(o);
    free(dst); free(buf); free(uin); free(pin); free(pinf); free(tail0); free(tail); free(u); free(mapped); free(sums); free(cleared);
    return 0;
}
