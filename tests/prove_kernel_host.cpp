// prove_kernel_host.cpp -- the kernels of zkvm_pairings_amd/csrc/zkp_prove.hip (k_spmv, k_prove_sat_init, k_prove_sat, k_prove_quot,
// k_prove_rs, k_prove_pad, k_prove_bcast, k_prove_mulinf) compiled for the HOST and run as written: one std::thread per lane of a workgroup, a pthread barrier for
// __syncthreads, the workgroups one after the other, `__shared__` as a static array.  tests/test_prove_cpu.py builds this with
// g++ -fsanitize=address,undefined, runs it as a child process and compares what the kernels leave with tests/prove_model.py and
// Python integers, byte for byte.  Every array is a std::vector of exactly the size the ABI promises, so a read outside a matrix's
// arrays - a malformed matrix is among the inputs - is an AddressSanitizer report.  The grids are repeated here from fr_spmv and the
// drivers in zkp_prove.hip.  CPU only: nothing here touches HIP.
//
//   prove_kernel_host spmv <in> <out> <n_rows> <n_cols> <nnz> <n> <out_stride> <t or -1> <brv_log2>
//        in: row_ptr (n_rows + 1 u32) | col (nnz u32) | val (nnz x 32 B) | x (n x n_cols x 32 B); out: n x out_stride x 32 B | flag (4 B);
//        the output is pre-filled with ones
//   prove_kernel_host quot <in> <out> <log2_n> <n>      in: a | b | c (n N each); out: sat of (a, b, c) (n bytes) | the quotient kernel's a
//   prove_kernel_host rs   <in> <out> <n>               in: rs (n x 64 B); out: r | s | -r s
//   prove_kernel_host pad  <in> <out> <n_src> <lead> <total> <with_inf>   in: src (n_src x 96 B) [| inf (n_src)]; out: dst (total x 96 B) | dst_inf
//   prove_kernel_host bcast  <in> <out> <words> <n>      in: one point of `words` u64; out: n copies
//   prove_kernel_host mulinf <in> <out> <n>              in: base_inf (n) | out (n x 96 B) | out_inf (n); out: out | out_inf after the kernel
#include <pthread.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#define ZKP_PROVE_KERNELS_ONLY
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
struct D3 { unsigned x, y; };
static thread_local D3 threadIdx, blockIdx, blockDim, gridDim;
static pthread_barrier_t g_bar;
static void __syncthreads() { pthread_barrier_wait(&g_bar); }
static int atomicOr(int* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
#include "../zkvm_pairings_amd/csrc/zkp_prove.hip"

using namespace zkp;
template <class F> static void launch(unsigned gx, unsigned gy, unsigned block, F f) {
    for (unsigned by = 0; by < gy; by++)
        for (unsigned b = 0; b < gx; b++) {
            pthread_barrier_init(&g_bar, nullptr, block);
            std::vector<std::thread> th;
            for (unsigned t = 0; t < block; t++)
                th.emplace_back([=] { threadIdx.x = t; threadIdx.y = 0; blockIdx.x = b; blockIdx.y = by; blockDim.x = block; blockDim.y = 1; gridDim.x = gx; gridDim.y = gy; f(); });
            for (auto& x : th) x.join();
            pthread_barrier_destroy(&g_bar);
        }
}
template <class T> static bool take(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <class T> static void give(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const std::string mode = argv[1];
    FILE* fi = fopen(argv[2], "rb");
    if (!fi) return 3;
    FILE* fo = nullptr;
    auto arg = [&](int i) { return (size_t)strtoull(argv[i], nullptr, 10); };
    if (mode == "spmv" && argc >= 11) {
        const size_t n_rows = arg(4), n_cols = arg(5), nnz = arg(6), n = arg(7), out_stride = arg(8);
        const int t_arg = atoi(argv[9]);
        const unsigned brv = (unsigned)arg(10);
        std::vector<uint32_t> row_ptr(n_rows + 1), col(nnz);
        std::vector<uint64_t> val(4 * nnz), x(4 * n * n_cols), out(4 * n * out_stride, 1);
        if (!take(fi, row_ptr) || !take(fi, col) || !take(fi, val) || !take(fi, x)) return 3;
        prove::SpmvGrid g = prove::spmv_grid(nnz, n_rows, n, out_stride);
        if (t_arg >= 0) {   // exact arithmetic: any lane count gives the same bytes
            g.t = (unsigned)t_arg;
            const size_t per = prove::TPB >> g.t;
            g.x = (unsigned)((out_stride + per - 1) / per);
        }
        int bad = 0;
        if (n && out_stride)
            launch(g.x, g.y, prove::TPB, [&] {
                k_spmv(row_ptr.data(), col.data(), val.data(), x.data(), out.data(), (uint32_t)n_rows, (uint32_t)n_cols, (uint32_t)nnz, (uint32_t)n,
                       (uint32_t)out_stride, g.t, brv, &bad);
            });
        fo = fopen(argv[3], "wb");
        give(fo, out);
        fwrite(&bad, 4, 1, fo);
    } else if (mode == "quot" && argc >= 6) {
        constexpr fr::Consts K = fr::make_consts();
        const unsigned k = (unsigned)arg(4);
        const size_t n = arg(5), total = n << k;
        std::vector<uint64_t> a(4 * total), b(4 * total), c(4 * total);
        std::vector<uint8_t> sat(n, 7);
        if (!take(fi, a) || !take(fi, b) || !take(fi, c)) return 3;
        launch((unsigned)((n + 255) / 256), 1, 256, [&] { k_prove_sat_init(sat.data(), (uint32_t)n); });
        launch((unsigned)((total + 255) / 256), 1, 256, [&] { k_prove_sat(a.data(), b.data(), c.data(), (uint32_t)total, k, sat.data()); });
        FrK kinv;   // (7^N - 1)^-1 in Montgomery form, as coset_vanishing_inverse in zkp_prove.hip
        const uint32_t seven[8] = {7};
        fr::to_mont(kinv.w, seven);
        for (unsigned i = 0; i < k; i++) fr::mont_mul(kinv.w, kinv.w, kinv.w);
        fr::sub(kinv.w, kinv.w, K.one);
        fr::mont_inv(kinv.w, kinv.w);
        launch((unsigned)((total + 255) / 256), 1, 256, [&] { k_prove_quot(a.data(), b.data(), c.data(), (uint32_t)total, kinv); });
        fo = fopen(argv[3], "wb");
        give(fo, sat);
        give(fo, a);
    } else if (mode == "rs") {
        const size_t n = arg(4);
        std::vector<uint64_t> rs(8 * n), r(4 * n), s(4 * n), nrs(4 * n);
        if (!take(fi, rs)) return 3;
        launch((unsigned)((n + 255) / 256), 1, 256, [&] { k_prove_rs(rs.data(), (uint32_t)n, r.data(), s.data(), nrs.data()); });
        fo = fopen(argv[3], "wb");
        give(fo, r);
        give(fo, s);
        give(fo, nrs);
    } else if (mode == "pad" && argc >= 8) {
        const size_t n_src = arg(4), lead = arg(5), total = arg(6), with_inf = arg(7);
        std::vector<uint64_t> src(12 * n_src), dst(12 * total, 5);
        std::vector<uint8_t> inf(with_inf ? n_src : 0), dst_inf(total, 9);
        if (!take(fi, src) || !take(fi, inf)) return 3;
        launch((unsigned)((total + 255) / 256), 1, 256, [&] {
            k_prove_pad(n_src ? src.data() : nullptr, with_inf && n_src ? inf.data() : nullptr, (uint32_t)n_src, (uint32_t)lead, (uint32_t)total, dst.data(),
                        dst_inf.data());
        });
        fo = fopen(argv[3], "wb");
        give(fo, dst);
        give(fo, dst_inf);
    } else if (mode == "bcast" && argc >= 6) {
        const size_t words = arg(4), n = arg(5);
        std::vector<uint64_t> pt(words), out(words * n, 3);
        if (!take(fi, pt)) return 3;
        launch((unsigned)((n * words + 255) / 256), 1, 256, [&] { k_prove_bcast(pt.data(), (uint32_t)words, (uint32_t)n, out.data()); });
        fo = fopen(argv[3], "wb");
        give(fo, out);
    } else if (mode == "mulinf") {
        const size_t n = arg(4);
        std::vector<uint8_t> base_inf(n), out_inf(n);
        std::vector<uint64_t> out(12 * n);
        if (!take(fi, base_inf) || !take(fi, out) || !take(fi, out_inf)) return 3;
        launch((unsigned)((n + 255) / 256), 1, 256, [&] { k_prove_mulinf(base_inf.data(), (uint32_t)n, out.data(), out_inf.data()); });
        fo = fopen(argv[3], "wb");
        give(fo, out);
        give(fo, out_inf);
    } else {
        return 2;
    }
    fclose(fi);
    fclose(fo);
    return 0;
}
