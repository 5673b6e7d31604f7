// grp_kernel_host.cpp -- the index kernels of zkvm_pairings_amd/csrc/zkp_bls_grouped.hip (k_grp_check: the offsets, the statuses, the
// call's word; k_grp_keys: the bounded search of a signature's group and the flag of a real contribution) compiled for the HOST and run as
// written, in the manner of tests/agg_kernel_host.cpp: the lanes of a launch one after the other.  tests/test_grp_cpu.py builds this with
// g++ -fsanitize=address,undefined, runs it as a child process and compares what the kernels leave with tests/grp_model.py.  Every buffer
// is allocated EXACTLY (n keys, n_seg + 1 offsets, n_seg statuses): a load that follows a bad offset out of its array is a sanitizer
// report.  CPU only: nothing here touches HIP.
//
//   grp_kernel_host <in> <out>
//   in:  u64 n | u64 n_seg | seg_off (n_seg + 1 u64)
//   out: keys (n u32) | status (n_seg bytes) | the call's word (4 B) | the validation word (4 B)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define ZKP_GRP_KERNELS_ONLY
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct D3 { unsigned x; };
static D3 threadIdx, blockIdx;
static int atomicOr(int* p, int v) {
    const int old = *p;
    *p |= v;
    return old;
}
#include "../zkvm_pairings_amd/csrc/zkp_bls_grouped.hip"

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
static void* exact(size_t bytes) { return malloc(bytes ? bytes : 1); }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hd[2];
    if (fread(hd, 8, 2, f) != 2) return 2;
    const uint64_t n = hd[0], n_seg = hd[1];
    if (grp::args_bad(n, n_seg) || n > (1u << 20) || n_seg > (1u << 20)) return 2;
    uint64_t* seg_off = (uint64_t*)exact(8 * (n_seg + 1));
    if (fread(seg_off, 8, n_seg + 1, f) != n_seg + 1) return 2;
    fclose(f);

    uint32_t* keys = (uint32_t*)exact(4 * n);
    uint8_t* status = (uint8_t*)exact(n_seg);
    memset(keys, 0xEE, 4 * n);
    memset(status, 0xEE, n_seg);
    int word = 0, bad = 0;                                               // k_grp_zero's part
    launch((unsigned)((n_seg + 1 + TPB_I - 1) / TPB_I), TPB_I, [&] { k_grp_check(seg_off, (uint32_t)n_seg, n, status, &word, &bad); });
    if (n) launch((unsigned)((n + TPB_I - 1) / TPB_I), TPB_I, [&] { k_grp_keys((uint32_t)n, seg_off, (uint32_t)n_seg, &word, keys); });

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(keys, 4, n, o);
    fwrite(status, 1, n_seg, o);
    const int32_t w[2] = {word, bad};
    fwrite(w, 4, 2, o);
    fclose(o);
    free(seg_off); free(keys); free(status);
    return 0;
}
