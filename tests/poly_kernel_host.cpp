// poly_kernel_host.cpp -- the kernels of zkvm_pairings_amd/csrc/zkp_poly.hip (k_ntt_pass in both decimations, k_poly_coset, k_open_quot)
// compiled for the HOST and run as written: one std::thread per lane of a workgroup, a pthread barrier for __syncthreads, the workgroups
// one after the other, `__shared__` as a static array.  tests/test_poly_cpu.py builds this with g++ -fsanitize=address,undefined, runs it
// as a child process and compares what the kernels leave with tests/poly_model.py and Python integers, byte for byte.  It is what a
// machine without a GPU can say about the device code itself; the launches (grids, pass order, buffers) are repeated here from
// fr_ntt in zkp_poly.hip.  CPU only: nothing here touches HIP.
//
//   poly_kernel_host ntt  <in> <out> <log2_n> <n_poly> <flags> [inplace]     in: n_poly << log2_n elements of 32 bytes
//   poly_kernel_host quot <in> <out> <log2_n> <n> <bitrev>                    in: evals (n N) | y (n) | 1 / (z - w^i) (n N); out: q
#include <pthread.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#define ZKP_POLY_KERNELS_ONLY
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
struct D3 { unsigned x; };
static thread_local D3 threadIdx, blockIdx, blockDim;
static pthread_barrier_t g_bar;
static void __syncthreads() { pthread_barrier_wait(&g_bar); }
#include "../zkvm_pairings_amd/csrc/zkp_poly.hip"

using namespace zkp;
template <class F> static void launch(unsigned grid, unsigned block, F f) {
    for (unsigned b = 0; b < grid; b++) {
        pthread_barrier_init(&g_bar, nullptr, block);
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block; t++) th.emplace_back([=] { threadIdx.x = t; blockIdx.x = b; blockDim.x = block; f(); });
        for (auto& x : th) x.join();
        pthread_barrier_destroy(&g_bar);
    }
}
int main(int argc, char** argv) {
    if (argc < 7) return 2;
    constexpr fr::Consts K = fr::make_consts();
    constexpr fr::Roots W = fr::make_roots();
    const std::string mode = argv[1];
    const unsigned k = atoi(argv[4]), tl = 14;
    std::vector<uint32_t> table((size_t)8 << tl);
    memcpy(&table[0], K.one, 32);
    for (size_t i = 1; i < ((size_t)1 << tl); i++) fr::mont_mul(&table[8 * i], &table[8 * (i - 1)], W.omega[tl]);
    FILE* fi = fopen(argv[2], "rb");
    if (mode == "ntt") {
        const unsigned n_poly = atoi(argv[5]); const int flags = atoi(argv[6]);
        const size_t total = (size_t)n_poly << k;
        std::vector<uint64_t> in(4 * total), out(4 * total), ws(4 * total);
        if (fread(in.data(), 32, total, fi) != total) return 3;
        std::vector<uint32_t> coset(4 * 1024 * 8);
        {
            const uint32_t seven[8] = {7};
            FrWords g[4];
            fr::to_mont(g[0].w, seven); fr::mont_inv(g[2].w, g[0].w);
            for (int which = 0; which < 4; which += 2) { g[which + 1] = g[which]; for (int i = 0; i < 10; i++) fr::mont_mul(g[which + 1].w, g[which + 1].w, g[which + 1].w); }
            launch(16, 256, [&] { k_poly_coset(coset.data(), g[0], g[1], g[2], g[3]); });
        }
        const poly::Plan P = poly::make_plan(n_poly, k, flags);
        const unsigned grid = (unsigned)poly::ntt_tiles(n_poly, k);
        FrWords ninv = words_of(W.inv_pow2[k]);
        const bool inplace = argc > 7;
        for (int p = 0; p < P.n_pass; p++) {
            const bool last = p == P.n_pass - 1;
            uint64_t* o = inplace ? in.data() : out.data();
            uint64_t* mid = P.workspace ? ws.data() : o;
            const uint64_t* src = p == 0 ? in.data() : mid;
            uint64_t* dst = last ? o : mid;
            const poly::Pass a = P.pass[p];
            if (a.dit) launch(grid, 256, [&] { k_ntt_pass<true>(src, dst, table.data(), tl - k, coset.data(), a, ninv); });
            else launch(grid, 256, [&] { k_ntt_pass<false>(src, dst, table.data(), tl - k, coset.data(), a, ninv); });
        }
        FILE* fo = fopen(argv[3], "wb");
        fwrite(inplace ? in.data() : out.data(), 32, total, fo); fclose(fo);
    } else {   // quot: file holds evals (n*N), y (n), dinv (n*N)
        const unsigned n = atoi(argv[5]); const int bitrev = atoi(argv[6]);
        const size_t total = (size_t)n << k;
        std::vector<uint64_t> ev(4 * total), y(4 * n), q(4 * total);
        if (fread(ev.data(), 32, total, fi) != total || fread(y.data(), 32, n, fi) != n || fread(q.data(), 32, total, fi) != total) return 3;
        const unsigned tp_log2 = k < 8 ? k : 8, per = 256 >> tp_log2;
        launch((n + per - 1) / per, 256, [&] { k_open_quot(ev.data(), y.data(), q.data(), table.data(), tl - k, k, bitrev, n, tp_log2); });
        FILE* fo = fopen(argv[3], "wb");
        fwrite(q.data(), 32, total, fo); fclose(fo);
    }
    return 0;
}
