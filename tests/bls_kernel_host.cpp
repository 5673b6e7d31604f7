// bls_kernel_host.cpp -- the hash kernels of zkvm_pairings_amd/csrc/zkp_bls.hip (k_h2c_tails, k_h2f, k_h2c_wide: SHA-256 with its rolling
// schedule, expand_message_xmd, the dword / byte / tail loads of the messages, the wide reduction on the 28-bit core) compiled for the
// HOST and run as written, in the manner of tests/recover_kernel_host.cpp: the lanes of a launch one after the other.
// tests/test_h2c_cpu.py builds this with g++ -fsanitize=address,undefined, runs it as a child process and compares what the kernels
// leave with tests/h2c_model.py, byte for byte.  Every buffer is allocated EXACTLY (the messages end where the last offset says, the two
// tails have the lengths the planner gives): a load past an unaligned tail is a sanitizer report.  CPU only: nothing here touches HIP.
//
//   bls_kernel_host <in> <out>
//   in:  u64 dst_len | u64 n | u64 n_wide | u64 base | dst | offsets (n + 1 u64, absolute: the first is base) | the bytes
//        [base, offsets[n]) | n_wide x 64 bytes
//   out: u (n x 192 B) | the wide reductions (n_wide x 48 B) | the validation word (4 B)
// base > 0: the kernel gets the pointer of byte `base` minus base, as the host flavour of the library biases its staged copy - offsets
// near 2^40 index it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define ZKP_BLS_KERNELS_ONLY
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
#include "../zkvm_pairings_amd/csrc/zkp_bls.hip"

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

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hd[4];
    if (fread(hd, 8, 4, f) != 4) return 2;
    const uint64_t dst_len = hd[0], n = hd[1], n_wide = hd[2], base = hd[3];
    if (bls::dst_bad(dst_len) || n > 4096 || n_wide > 4096) return 2;
    uint8_t* dst = exact(dst_len);
    std::vector<uint64_t> offsets(n + 1);
    if (fread(dst, 1, dst_len, f) != dst_len || fread(offsets.data(), 8, n + 1, f) != n + 1) return 2;
    // offsets may decrease in between (the kernel must not follow them): the buffer holds [base, the largest offset that is sound)
    const uint64_t end = offsets[n] >= base ? offsets[n] : base;
    const size_t buf_len = (size_t)(end - base);
    uint8_t* buf = exact(buf_len);
    if (fread(buf, 1, buf_len, f) != buf_len) return 2;
    uint8_t* wide = exact(64 * n_wide);
    if (fread(wide, 1, 64 * n_wide, f) != 64 * n_wide) return 2;
    fclose(f);

    uint8_t* tail0 = exact(dst_len + 4);
    uint32_t* tail = (uint32_t*)exact(bls::tail_words(dst_len) * 4);
    uint64_t* u = (uint64_t*)exact(n * 192);
    uint64_t* red = (uint64_t*)exact(n_wide * 48);
    int bad = 0;
    // the biased pointer of the host flavour (stage_msgs): integer arithmetic, the kernel adds the offset back
    const uint8_t* msgs = (const uint8_t*)((uintptr_t)buf - (uintptr_t)base);
    launch(1, 1, [&] { k_h2c_tails(dst, (uint32_t)dst_len, tail0, tail); });
    if (n) launch((unsigned)((n + TPB_H - 1) / TPB_H), TPB_H, [&] { k_h2f(msgs, offsets.data(), 0, (uint32_t)n, n, tail0, tail, (uint32_t)dst_len, u, &bad); });
    if (n_wide) launch((unsigned)((n_wide + TPB_H - 1) / TPB_H), TPB_H, [&] { k_h2c_wide(wide, n_wide, red); });

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(u, 1, n * 192, o);
    fwrite(red, 1, n_wide * 48, o);
    const int32_t word = bad;
    fwrite(&word, 4, 1, o);
    fclose(o);
    free(dst); free(buf); free(wide); free(tail0); free(tail); free(u); free(red);
    return 0;
}
