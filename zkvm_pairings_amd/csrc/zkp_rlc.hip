// zkp_rlc.hip -- n independent pairing checks verified as ONE by a random linear combination (zkp_pairing_check_batch_rlc):
//
//     prod_c ( prod_j e(P_cj, Q_cj) )^(r_c) == 1,   r_c = a_c + b_c z^2,  (a_c, b_c) 64-bit random
//
// with one final exponentiation.  The exponent goes onto the G1 side: free pairs (P_cj, Q_cj) become ([r_c] P_cj, Q_cj) (k_g1_mul_endo28,
// 64 doublings through the endomorphism); a column of pairs (col_g1[c][j], fixed_g2[j]) becomes ONE pair (sum_c [r_c] col_g1[c][j],
// fixed_g2[j]) through a G1 MSM, and a column (fixed_g1[j], col_g2[c][j]) one pair (fixed_g1[j], sum_c [r_c] col_g2[c][j]) through a G2 MSM.
//   1. points   unless ZKP_RLC_POINTS_CHECKED: is_valid of every input point, statuses folded into one device flag
//   2. scalars  r_c as 4-word integers for the MSMs, `cols` copies; a zero (a, b) clears the flag      k_rlc_scalars
//   3. scale    the free G1 points, k per (a, b)                                                      coop_g1_mul_endo
//   4. columns  col_g1 / col_g2 to column-major order, s2 G1 and s1 G2 sums, the fixed points beside them    k_rlc_transpose, msm_run
//   5. pairing  one Miller product over the scaled free pairs, one over the s1 + s2 column pairs, their product, one final exponentiation
//   6. result   all_ok = (product == 1) AND every point valid AND no zero scalar                     k_rlc_finish
// Sizes come from zkp_rlc_plan.hpp; every launch is queued on the caller's stream: no read-back, and no allocation once the workspaces
// have reached the call's size (capturable into a hipGraph).
#include "zkp_rlc.hpp"

#include "zkp_coop.hpp"
#include "zkp_msm.hpp"
#include "zkp_rlc_plan.hpp"

namespace zkp {
namespace {

__global__ void k_rlc_init(int* flag, int* all_ok, int n_zero) {
    if (n_zero) { *all_ok = 1; return; }
    flag[0] = 1;
    flag[1] = 0;
}
// any non-zero status byte clears flag[0] (every writer writes the same 0: a plain store)
__global__ void k_rlc_fold(const uint8_t* st, size_t n, int* flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && st[i]) flag[0] = 0;
}
// sc[(j n + c) 4 ..] = a_c + b_c z^2 for j < cols; a zero scalar would drop its check: it clears flag[0]
__global__ void k_rlc_scalars(const uint64_t* rand, size_t n, size_t cols, uint64_t* sc, int* flag) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const uint64_t a = rand[2 * c], b = rand[2 * c + 1];
    if (!a && !b) flag[0] = 0;
    uint64_t r[rlc::SCALAR_U64];
    rlc::scalar(a, b, r);
    for (size_t j = 0; j < cols; j++)
        for (size_t w = 0; w < rlc::SCALAR_U64; w++) sc[(j * n + c) * rlc::SCALAR_U64 + w] = r[w];
}
// row-major n x s points (words u64 each) -> column-major s x n; infinity bytes alongside (iinf may be null)
__global__ void k_rlc_transpose(const uint64_t* in, const uint8_t* iinf, size_t n, size_t s, size_t words, uint64_t* out, uint8_t* oinf) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * s * words) return;
    const size_t pt = i / words, w = i - pt * words, c = pt / s, j = pt - c * s;
    out[(j * n + c) * words + w] = in[i];
    if (iinf && w == 0) oinf[j * n + c] = iinf[pt];
}
__global__ void k_rlc_finish(const int* flag, int* all_ok) { *all_ok = (flag[0] && flag[1]) ? 1 : 0; }

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int rlc_check_dev(zkp_ctx* c, const zkp_rlc_batch* b, const uint64_t* rand, int flags, int* all_ok, hipStream_t s) {
    const size_t n = b->n_checks, k = b->k, s1 = b->s1, s2 = b->s2;
    int rc;
    if (!n) {
        hipLaunchKernelGGL(k_rlc_init, dim3(1), dim3(1), 0, s, (int*)nullptr, all_ok, 1);
        return ctxop::fail(c, "k_rlc_init", hipGetLastError());
    }
    const bool check = !(flags & ZKP_RLC_POINTS_CHECKED);
    const rlc::Layout L = rlc::make_layout(n, k, s1, s2, check);
    // every workspace first (an allocation synchronises the device): nothing below this block allocates
    void* ws = nullptr;
    if ((rc = ctxop::grow_rlc(c, L.total, &ws))) return rc;
    if (s1 || s2) {
        const size_t b1 = s2 ? msm_workspace_bytes(1, n, L.cols, 0) : 0, b2 = s1 ? msm_workspace_bytes(2, n, L.cols, 0) : 0;
        if ((rc = ctxop::grow_msm(c, b1 > b2 ? b1 : b2))) return rc;
    }
    char* w = (char*)ws;
    int* flag = (int*)(w + L.flag);
    uint8_t* st = (uint8_t*)(w + L.st);
    uint64_t* sc = (uint64_t*)(w + L.sc);
    uint64_t *mg1 = (uint64_t*)(w + L.mg1), *mg2 = (uint64_t*)(w + L.mg2), *ml = (uint64_t*)(w + L.ml);
    uint8_t *minf1 = (uint8_t*)(w + L.minf1), *minf2 = (uint8_t*)(w + L.minf2);
    const uint8_t *inf1 = (const uint8_t*)b->inf1, *inf2 = (const uint8_t*)b->inf2;

    hipLaunchKernelGGL(k_rlc_init, dim3(1), dim3(1), 0, s, flag, all_ok, 0);
    if ((rc = ctxop::fail(c, "k_rlc_init", hipGetLastError()))) return rc;
    // 1. the points check: statuses of all six arrays side by side, then one fold
    if (check) {
        uint8_t* at = st;
        auto valid = [&](int which, const void* pts, const void* inf, size_t cnt) -> int {
            if (!cnt) return ZKP_OK;
            const int r = ctxop::valid(c, which, pts, inf, cnt, at, s);
            at += cnt;
            return r;
        };
        if ((rc = valid(1, b->g1, b->inf1, n * k)) || (rc = valid(2, b->g2, b->inf2, n * k)) || (rc = valid(1, b->col_g1, b->col_inf1, n * s2)) ||
            (rc = valid(2, b->fixed_g2, b->fixed_inf2, s2)) || (rc = valid(2, b->col_g2, b->col_inf2, n * s1)) ||
            (rc = valid(1, b->fixed_g1, b->fixed_inf1, s1)))
            return rc;
        hipLaunchKernelGGL(k_rlc_fold, dim3(blocks(L.n_status)), dim3(256), 0, s, st, L.n_status, flag);
        if ((rc = ctxop::fail(c, "k_rlc_fold", hipGetLastError()))) return rc;
    }
    // 2. the scalars (also what flags a zero (a, b))
    hipLaunchKernelGGL(k_rlc_scalars, dim3(blocks(n)), dim3(256), 0, s, rand, n, L.cols, sc, flag);
    if ((rc = ctxop::fail(c, "k_rlc_scalars", hipGetLastError()))) return rc;
    size_t nrec = 0;
    // 3. + 5a. the free pairs: [r_c] P_cj, then their Miller product
    if (k) {
        uint64_t* sg1 = (uint64_t*)(w + L.sg1);
        uint8_t* sinf = (uint8_t*)(w + L.sinf);
        if ((rc = ctxop::fail(c, "g1_mul_endo", coop_g1_mul_endo((const uint64_t*)b->g1, inf1, rand, n * k, (uint32_t)k, sg1, sinf, s))) ||
            (rc = ctxop::miller_product(c, sg1, (const uint64_t*)b->g2, sinf, inf2, n * k, ml + 72 * nrec++, s)))
            return rc;
    }
    // 4. + 5b. the columns: one MSM per `cols` columns, sums and fixed points side by side as s2 + s1 pairs
    auto columns = [&](int which, const void* col, const void* col_inf, size_t cnt, size_t words, uint64_t* t, uint8_t* tinf, uint64_t* sums,
                       uint8_t* sums_inf) -> int {
        hipLaunchKernelGGL(k_rlc_transpose, dim3(blocks(n * cnt * words)), dim3(256), 0, s, (const uint64_t*)col, (const uint8_t*)col_inf, n, cnt,
                           words, t, tinf);
        int r = ctxop::fail(c, "k_rlc_transpose", hipGetLastError());
        for (size_t j0 = 0; j0 < cnt && !r; j0 += L.cols) {
            const size_t m = cnt - j0 < L.cols ? cnt - j0 : L.cols;
            r = ctxop::msm(c, which, t + j0 * n * words, col_inf ? tinf + j0 * n : nullptr, sc, n, m, sums + j0 * words, sums_inf + j0, s);
        }
        return r;
    };
    auto place = [&](void* dst, uint8_t* dinf, const void* src, const void* sinf, size_t cnt, size_t words) -> int {
        int r = ctxop::fail(c, "hipMemcpyAsync (rlc fixed points)", hipMemcpyAsync(dst, src, cnt * words * 8, hipMemcpyDeviceToDevice, s));
        if (!r)
            r = ctxop::fail(c, "rlc fixed infinity flags", sinf ? hipMemcpyAsync(dinf, sinf, cnt, hipMemcpyDeviceToDevice, s) : hipMemsetAsync(dinf, 0, cnt, s));
        return r;
    };
    if (s2 && ((rc = columns(1, b->col_g1, b->col_inf1, s2, 12, (uint64_t*)(w + L.tg1), (uint8_t*)(w + L.tinf1), mg1, minf1)) ||
               (rc = place(mg2, minf2, b->fixed_g2, b->fixed_inf2, s2, 24))))
        return rc;
    if (s1 && ((rc = columns(2, b->col_g2, b->col_inf2, s1, 24, (uint64_t*)(w + L.tg2), (uint8_t*)(w + L.tinf2), mg2 + 24 * s2, minf2 + s2)) ||
               (rc = place(mg1 + 12 * s2, minf1 + s2, b->fixed_g1, b->fixed_inf1, s1, 12))))
        return rc;
    if ((s1 || s2) && (rc = ctxop::miller_product(c, mg1, mg2, minf1, minf2, s1 + s2, ml + 72 * nrec++, s))) return rc;
    // 5c. + 6. one final exponentiation of the product, then the AND
    if ((rc = ctxop::gt_is_one(c, ml, nrec, ml + 72 * (rlc::ML_RECORDS - 1), flag + 1, s))) return rc;
    hipLaunchKernelGGL(k_rlc_finish, dim3(1), dim3(1), 0, s, flag, all_ok);
    return ctxop::fail(c, "k_rlc_finish", hipGetLastError());
}

}  // namespace zkp
