// zkp_msm.hip -- multi-scalar multiplication by the bucket method (Pippenger), G1 and G2 from one driver.
//
// Per pass (whole segments, zkp_msm_plan.hpp):
//   1. points   the pass's points (every point once when the bases are shared) to Montgomery records        k_msm_points
//   2. digits   signed c-bit windows of every scalar: one 32-bit key (bucket) + one value (point, sign) each  k_msm_digits
//   3. sort     radix sort of the pairs by key, low key_bits bits only (rocPRIM through hipCUB)
//   4. buckets  run-wise segmented sums, RUN sorted entries per lane with mixed additions; runs that cross a
//               bucket border leave partial sums that the next levels join with full additions                k_msm_accum
//   5. reduce   sum_j (j + 1) B_j per window with running sums, split over lanes; the chunk sums are joined
//               into window sums by the same segmented sum                                                    k_msm_reduce, k_msm_accum
//   6. final    Horner over the windows (c doublings each), one inversion per segment, affine wire output       k_msm_final
// Everything is enqueued on the caller's stream with sizes the host knows in advance: no read-back, no allocation.
#include "zkp_msm.hpp"

#include <hipcub/hipcub.hpp>

#include "zkp_coop.hpp"
#include "zkp_msm_plan.hpp"

namespace zkp {
namespace {

size_t sort_temp_bytes(uint32_t keys) {
    size_t bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (int)keys, 0, 32) != hipSuccess)
        return 0;
    return bytes;
}

// The bucket and window sums are zeroed by a kernel, where msm_run used to call hipMemsetAsync.  Observed on an MI355X: an MSM captured
// into a hipGraph with the two memset nodes gave the right sums on the first replay and wrong ones on every later replay (G1, 1 to 127
// terms and two sums of 1 to 65 terms, twelve replays each; eager calls and first replays were always right - DESIGN section 3.2).  With
// the fill kernel every replay is right.  The earlier graph tests replay once, so they never saw it; the Groth16 verifier's test
// replays twice.  bytes is a multiple of 16 (whole records), p 16-byte aligned.
__global__ void k_zero_fill(uint4* p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = make_uint4(0, 0, 0, 0);
}
inline hipError_t zero_fill(void* p, size_t bytes, hipStream_t s) {
    const size_t n16 = bytes / 16;
    if (!n16) return hipSuccess;
    const size_t want = (n16 + 255) / 256;
    hipLaunchKernelGGL(k_zero_fill, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, s, (uint4*)p, n16);
    return hipGetLastError();
}

}  // namespace

size_t msm_workspace_bytes(int which, size_t m, size_t n_msm, int shared) {
    msm::Plan p;
    if (!msm::make_plan(m, n_msm, shared != 0, &p)) return 0;
    return msm::make_layout(p, which == 1 ? 2 : 4, sort_temp_bytes(p.keys)).total;
}

hipError_t msm_run(int which, void* ws, const uint64_t* points, const uint8_t* inf, const uint64_t* scalars, size_t m, size_t n_msm, int shared,
                   uint64_t* out, uint8_t* out_inf, hipStream_t s, float* phase_ms) {
    msm::Plan p;
    if (!msm::make_plan(m, n_msm, shared != 0, &p)) return n_msm ? hipErrorInvalidValue : hipSuccess;
    const uint32_t np = which == 1 ? 2 : 4, pw = 6 * np;   // Fp per point, u64 per point
    const size_t jr = (size_t)3 * (np / 2) * msm::REC_BYTES;
    size_t temp = sort_temp_bytes(p.keys);
    const msm::Layout L = msm::make_layout(p, np, temp);
    char* b = (char*)ws;
    void* pts = b + L.pts;
    uint32_t *k_in = (uint32_t*)(b + L.keys_in), *v_in = (uint32_t*)(b + L.vals_in), *k_out = (uint32_t*)(b + L.keys_out),
             *v_out = (uint32_t*)(b + L.vals_out);
    uint32_t* part_k[2] = {(uint32_t*)(b + L.part_k[0]), (uint32_t*)(b + L.part_k[1])};
    void* part_j[2] = {b + L.part_j[0], b + L.part_j[1]};
    hipEvent_t ev[MSM_PHASES + 1] = {};
    hipError_t e = hipSuccess;
    if (phase_ms)
        for (int i = 0; i <= MSM_PHASES && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    auto mark = [&](int i) { if (phase_ms && e == hipSuccess) e = hipEventRecord(ev[i], s); };
#define MSM_CHK(x)                      \
    do {                                \
        if (e == hipSuccess) e = (x);   \
    } while (0)
    for (uint32_t pass = 0; pass < p.passes && e == hipSuccess; pass++) {
        const size_t seg0 = (size_t)pass * p.segs;
        const uint32_t segs = (uint32_t)(n_msm - seg0 < p.segs ? n_msm - seg0 : p.segs);
        const uint32_t terms = (uint32_t)(segs * m), keys = terms * p.windows;
        const size_t t0 = seg0 * m;
        mark(0);
        if (!shared || pass == 0) MSM_CHK(msm_points(points + (shared ? 0 : t0 * pw), (shared ? (uint32_t)m : terms) * np, pts, s));
        mark(1);
        MSM_CHK(msm_digits(scalars + 4 * t0, inf ? inf + (shared ? 0 : t0) : nullptr, terms, (uint32_t)m, shared, p.c, p.windows, k_in, v_in, s));
        mark(2);
        MSM_CHK(hipcub::DeviceRadixSort::SortPairs(b + L.sort_temp, temp, k_in, k_out, v_in, v_out, (int)keys, 0, (int)p.key_bits, s));
        mark(3);
        const uint32_t n_buckets = segs * p.windows * p.nb, n_sums = segs * p.windows;
        MSM_CHK(zero_fill(b + L.buckets, (size_t)n_buckets * jr, s));
        // level 0 from the sorted digits, then the partial sums ping-pong until one run is left
        uint32_t n = keys;
        const uint32_t* kin = k_out;
        const void* jin = pts;
        for (int lv = 0; e == hipSuccess; lv++) {
            MSM_CHK(msm_accum(which, lv == 0, kin, v_out, jin, n, n_buckets, b + L.buckets, part_k[lv & 1], part_j[lv & 1], s));
            if (n <= msm::RUN) break;
            n = 2 * msm::runs_of(n);
            kin = part_k[lv & 1];
            jin = part_j[lv & 1];
        }
        mark(4);
        MSM_CHK(msm_reduce(which, b + L.buckets, n_sums, p.split, p.chunk, (uint32_t*)(b + L.chunk_k), b + L.chunk_j, s));
        MSM_CHK(zero_fill(b + L.wsums, (size_t)n_sums * jr, s));
        n = n_sums * p.split;
        kin = (const uint32_t*)(b + L.chunk_k);
        jin = b + L.chunk_j;
        for (int lv = 0; e == hipSuccess; lv++) {
            MSM_CHK(msm_accum(which, false, kin, nullptr, jin, n, n_sums, b + L.wsums, part_k[lv & 1], part_j[lv & 1], s));
            if (n <= msm::RUN) break;
            n = 2 * msm::runs_of(n);
            kin = part_k[lv & 1];
            jin = part_j[lv & 1];
        }
        mark(5);
        MSM_CHK(msm_final(which, b + L.wsums, segs, p.windows, p.c, out + seg0 * pw, out_inf ? out_inf + seg0 : nullptr, s));
        mark(6);
        if (phase_ms && e == hipSuccess) {
            e = hipEventSynchronize(ev[MSM_PHASES]);
            for (int i = 0; i < MSM_PHASES && e == hipSuccess; i++) {
                float ms = 0;
                e = hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
                phase_ms[i] += ms;
            }
        }
    }
#undef MSM_CHK
    for (int i = 0; i <= MSM_PHASES; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    return e;
}

}  // namespace zkp
