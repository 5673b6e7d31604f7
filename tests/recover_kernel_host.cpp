// recover_kernel_host.cpp -- the kernels of zkvm_pairings_amd/csrc/zkp_recover.hip (k_rec_vanish, k_rec_zinv, k_rec_column) compiled for
// the HOST and run as written, in the manner of tests/poly_kernel_host.cpp: one std::thread per lane of a workgroup, a pthread barrier for
// __syncthreads, the workgroups one after the other, `__shared__` as a static array.  tests/test_recover_cpu.py builds this with
// g++ -fsanitize=address,undefined, runs it as a child process and compares what the kernels leave with tests/recover_model.py, byte for
// byte.  The launches (grids, arguments, the scale constant) are repeated here from recover_dev; what the driver gets from the Fr
// transform - the interpolants' coefficients, Z on the roots, Z on the coset - comes from the model, in the input file.  CPU only:
// nothing here touches HIP.
//
//   recover_kernel_host <in> <out> <log2_n> <log2_l> <n> <bitrev>
//   in:  present (n M bytes) | coef (n M l x 32 B) | Z on the roots (n M x 32 B) | Z on the coset (n M x 32 B)
//   out: zc (n M x 32 B) | ok after k_rec_vanish (n x 4 B) | 1 / Z on the coset after k_rec_zinv (n M x 32 B) | coefficients (n N x 32 B) |
//        ok after k_rec_column (n x 4 B)
#include <pthread.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#define ZKP_RECOVER_KERNELS_ONLY
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
#include "../zkvm_pairings_amd/csrc/zkp_recover.hip"

using namespace zkp;
template <class F> static void launch(unsigned grid, unsigned block, F f) {
    // the lanes' threads live for the whole launch (starting 256 of them per workgroup is most of a small workgroup's time); the barrier
    // behind a workgroup keeps a fast lane of the next one out of the `__shared__` arrays that a slow lane of this one still reads
    pthread_barrier_init(&g_bar, nullptr, block);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block; t++)
        th.emplace_back([=] {
            threadIdx.x = t;
            blockDim.x = block;
            for (unsigned b = 0; b < grid; b++) {
                blockIdx.x = b;
                f();
                pthread_barrier_wait(&g_bar);
            }
        });
    for (auto& x : th) x.join();
    pthread_barrier_destroy(&g_bar);
}
int main(int argc, char** argv) {
    if (argc < 7) return 2;
    constexpr fr::Consts K = fr::make_consts();
    constexpr fr::Roots W = fr::make_roots();
    const unsigned log2_n = atoi(argv[3]), log2_l = atoi(argv[4]), n = atoi(argv[5]);
    const int flags = atoi(argv[6]) ? poly::NTT_BITREV : 0;
    if (rec::args_bad(n, log2_n, log2_l, flags) || !n) return 2;
    const rec::Shape sh = rec::shape_of(log2_n, log2_l);
    const unsigned tl = sh.log2_d;
    std::vector<uint32_t> table((size_t)8 << tl);
    memcpy(&table[0], K.one, 32);
    for (size_t i = 1; i < ((size_t)1 << tl); i++) fr::mont_mul(&table[8 * i], &table[8 * (i - 1)], W.omega[tl]);
    std::vector<uint32_t> coset((size_t)4 * 8 << poly::COSET_LOG2);      // the kernels read 7^j and 7^-j, j < 2^10
    {
        const uint32_t seven[8] = {7};
        uint32_t g[8], gi[8];
        fr::to_mont(g, seven);
        fr::mont_inv(gi, g);
        for (int which = 0; which < 4; which += 2) {
            uint32_t* t = &coset[(size_t)which * 8 << poly::COSET_LOG2];
            memcpy(t, K.one, 32);
            for (size_t j = 1; j < ((size_t)1 << poly::COSET_LOG2); j++) fr::mont_mul(t + 8 * j, t + 8 * (j - 1), which ? gi : g);
        }
    }
    const size_t rows = (size_t)n << sh.mu, els = rows << log2_l, big_n = (size_t)n << log2_n;
    std::vector<uint8_t> present(rows);
    std::vector<uint64_t> coef(4 * els), zr(4 * rows), zsinv(4 * rows), zc(4 * rows), out(4 * big_n);
    std::vector<int32_t> ok(n, 7), ok_vanish;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi || fread(present.data(), 1, rows, fi) != rows || fread(coef.data(), 32, els, fi) != els || fread(zr.data(), 32, rows, fi) != rows ||
        fread(zsinv.data(), 32, rows, fi) != rows)
        return 3;
    fclose(fi);
    const rec::Column a = rec::column_of(log2_n, log2_l, flags, tl);
    FrWords scale;
    fr::mont_mul(scale.w, W.inv_pow2[2 * sh.mu], K.r2);
    fr::mont_mul(scale.w, scale.w, K.r2);
    launch(n, 256, [&] { k_rec_vanish(present.data(), table.data(), a.tshift_m, a.mu, a.bitrev, zc.data(), ok.data()); });
    ok_vanish = ok;
    const ZinvConsts& zk = zinv_consts();
    launch(n, 256, [&] { k_rec_zinv(present.data(), a.mu, zk.cinv[a.mu], zk.rpow[a.mu], zsinv.data()); });
    launch(n * sh.groups, 256, [&] { k_rec_column(coef.data(), present.data(), zr.data(), zsinv.data(), table.data(), coset.data(), a, scale, out.data(), ok.data()); });
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 3;
    fwrite(zc.data(), 32, rows, fo);
    fwrite(ok_vanish.data(), 4, n, fo);
    fwrite(zsinv.data(), 32, rows, fo);
    fwrite(out.data(), 32, big_n, fo);
    fwrite(ok.data(), 4, n, fo);
    fclose(fo);
    return 0;
}
