// agg_g2_kernel_host.cpp -- the expansion kernel of zkvm_pairings_amd/csrc/zkp_bls_agg_g2.hip (k_aggv_expand: a message's segment by the
// bounded search, its rand row, its signature or the flagged identity) behind the offset check it relies on (k_agg_check of
// zkp_bls_agg.hip), both compiled for the HOST and run as written, in the manner of tests/agg_kernel_host.cpp: the lanes of a launch one
// after the other.  tests/test_agg_g2_cpu.py builds this with g++ -fsanitize=address,undefined, runs it as a child process and compares
// what the kernels leave with tests/agg_g2_model.py.  Every buffer is allocated EXACTLY (n + 1 offsets, n signatures, n flags, n rand
// rows, n_msg output rows): a load that follows a bad offset out of its array is a sanitizer report.  CPU only: nothing here touches HIP.
//
//   agg_g2_kernel_host <in> <out>
//   in:  u64 n | u64 n_msg | u64 has_inf | seg_off (n + 1 u64) | sig (n x 24 u64) | rand (n x 2 u64) | inf_sig (n bytes, when has_inf)
//   out: x_sig (n_msg x 24 u64) | x_rand (n_msg x 2 u64) | x_inf (n_msg bytes) | status (n bytes) | the call's word (4 B) | the validation word (4 B)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define ZKP_AGG_KERNELS_ONLY
#define ZKP_AGG_G2_KERNELS_ONLY
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
#include "../zkvm_pairings_amd/csrc/zkp_bls_agg.hip"
#include "../zkvm_pairings_amd/csrc/zkp_bls_agg_g2.hip"

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
    uint64_t hd[3];
    if (fread(hd, 8, 3, f) != 3) return 2;
    const uint64_t n = hd[0], n_msg = hd[1], has_inf = hd[2];
    if (agg2::verify_args_bad(n_msg, n) || n_msg > (1u << 20) || n > (1u << 20)) return 2;
    uint64_t* seg_off = (uint64_t*)exact(8 * (n + 1));
    uint64_t* sig = (uint64_t*)exact(192 * n);
    uint64_t* rand = (uint64_t*)exact(16 * n);
    uint8_t* inf_sig = has_inf ? (uint8_t*)exact(n) : nullptr;
    if (fread(seg_off, 8, n + 1, f) != n + 1 || fread(sig, 192, n, f) != n || fread(rand, 16, n, f) != n || (has_inf && fread(inf_sig, 1, n, f) != n)) return 2;
    fclose(f);

    uint64_t *x_sig = (uint64_t*)exact(192 * n_msg), *x_rand = (uint64_t*)exact(16 * n_msg);
    uint8_t *x_inf = (uint8_t*)exact(n_msg), *status = (uint8_t*)exact(n);
    memset(x_sig, 0xEE, 192 * n_msg);
    memset(x_rand, 0xEE, 16 * n_msg);
    memset(x_inf, 0xEE, n_msg);
    memset(status, 0xEE, n);
    int word = 0, bad = 0;                                               // k_agg_zero's part
    launch((unsigned)((n + 1 + TPB_I - 1) / TPB_I), TPB_I, [&] { k_agg_check(seg_off, (uint32_t)n, n_msg, status, &word, &bad); });
    if (n_msg)
        launch((unsigned)((n_msg + TPB_X - 1) / TPB_X), TPB_X,
               [&] { k_aggv_expand(seg_off, (uint32_t)n, (uint32_t)n_msg, sig, inf_sig, rand, &word, x_sig, x_inf, x_rand); });

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(x_sig, 192, n_msg, o);
    fwrite(x_rand, 16, n_msg, o);
    fwrite(x_inf, 1, n_msg, o);
    fwrite(status, 1, n, o);
    const int32_t w[2] = {word, bad};
    fwrite(w, 4, 2, o);
    fclose(o);
    free(seg_off); free(sig); free(rand); free(inf_sig); free(x_sig); free(x_rand); free(x_inf); free(status);
    return 0;
}
