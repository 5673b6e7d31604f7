// zkp_recover.hip -- the cell recovery (zkp_das_recover_batch, include/zkp_recover.h): a blob back from any half of its cells.
//
// f(X) = sum_{i<l} X^i P_i(X^l): the interpolant of cell m is sum_i X^i P_i(w_M^m'), so column i of the interpolants' coefficients -
// the inverse size-l transform of a cell's values, coefficient i times c_m^-i - is the Reed-Solomon codeword of P_i (degree < k = M / 2)
// on the M-th roots of unity.  A blob is l erasure decodings of size M with ONE erasure pattern, hence one vanishing polynomial
// Z(Y) = prod over the missing m' of (Y - w_M^m').  A slice of blobs:
//   1. fr_ntt        inverse, size l, over the slice's M rows per blob, into the workspace (not for l = 1)
//   2. k_rec_vanish  a workgroup per blob: counts the present cells, multiplies Z up in LDS one linear factor at a time (canonical
//                    coefficients, zero-padded to M), writes ok = 1, or ok = 0 and Z = 0 when fewer than M / 2 cells are present
//   3. fr_ntt x 2    Z on the M-th roots and on the coset 7 w_M^t
//      k_rec_zinv    a workgroup per blob turns the second table into 1 / Z(7 w_M^t) in place WITHOUT a field inversion: the product of
//                    Z over the whole coset is (1 - 7^M)^deg Z (prod_t (7 w_M^t - a) = 1 - 7^M for every M-th root of unity a), so
//                    Montgomery's trick knows the inverse of its grand total beforehand - a power of a constant of the call - and what
//                    is left is two prefix-product scans in LDS, log2 M steps each.  (The batched inversion of zkp_kzg.hip spends
//                    0.55 ms in ONE thread's power r - 2, whatever the size: more than every other launch of this call together.)
//   4. k_rec_column  a workgroup per C consecutive columns of a blob, the columns in LDS from load to store: E[m'] Z(w_M^m') on load (0
//                    for a missing cell, whose bytes are not read), the inverse transform (q = P_i Z), 7^t and the forward transform
//                    (q on the coset), the product with 1 / Z, the inverse transform and 7^-t: p.  p_t is f_{i + l t} for t < k, and the
//                    cells are consistent iff p_t = 0 for every t >= k: a workgroup that sees a non-zero one stores ok = 0.
// The three transforms of a column alternate decimation in frequency and in time, so no permutation stands between them, and stay
// unscaled: the two products with canonical table entries (Z on the roots, 1 / Z on the coset) are Montgomery products that lose a
// factor R each, and ONE constant - 2^-2mu R^2, Montgomery form - repairs scale and form while storing.  Everything else follows
// k_ntt_pass: canonical data, Montgomery twiddles from the context's domain table, the tile word-major and folded (poly::lds_slot).
// A blob with too few cells has Z = 0 and a zero table in place of 1 / Z: its columns come out zero with no special case.  Exact; no
// atomics.
//
// tests/recover_kernel_host.cpp compiles the three kernels for the host (ZKP_RECOVER_KERNELS_ONLY: one std::thread per lane, a barrier for
// __syncthreads) and runs them under ASan and UBSan against the Python model; the launch code below the kernels is left out there.
#ifndef ZKP_RECOVER_KERNELS_ONLY
#include "zkp_recover.hpp"
#endif
#include "zkp_fr.hpp"
#include "zkp_recover_plan.hpp"

namespace zkp {
namespace {

using fr::NW;
constexpr int TPB = (int)poly::TPB;
constexpr uint32_t TILE = 1u << poly::TILE_LOG2;
static_assert(TILE == 4 * poly::TPB, "a thread holds four elements of the tile");

struct FrWords { uint32_t w[NW]; };

// the tile helpers of zkp_poly.hip, copied: that file's kernels keep their registers
__device__ __forceinline__ void tile_put(uint32_t* sh, uint32_t e, const uint32_t* v) {
    const uint32_t s = poly::lds_slot(e);
#pragma unroll
    for (int k = 0; k < NW; k++) sh[k * TILE + s] = v[k];
}
__device__ __forceinline__ void tile_get(uint32_t* v, const uint32_t* sh, uint32_t e) {
    const uint32_t s = poly::lds_slot(e);
#pragma unroll
    for (int k = 0; k < NW; k++) v[k] = sh[k * TILE + s];
}
__device__ __forceinline__ void table_get(uint32_t* v, const uint32_t* __restrict__ table, size_t at) {
#pragma unroll
    for (int k = 0; k < NW; k++) v[k] = table[at * NW + k];
}
// x <- x 7^i (inv = 0) or x 7^-i (inv = 1), i < 2^10: the low coset tables
__device__ __forceinline__ void coset_mul(uint32_t* x, const uint32_t* __restrict__ coset, uint32_t i, uint32_t inv) {
    uint32_t w[NW];
    table_get(w, coset, ((size_t)(2 * inv) << poly::COSET_LOG2) + i);
    fr::mont_mul(x, x, w);
}
template <bool DIT>
__device__ __forceinline__ void butterfly(uint32_t* a, uint32_t* b, const uint32_t* __restrict__ table, uint32_t tshift, uint32_t ti, bool has_twiddle) {
    uint32_t w[NW], d[NW];
    if (has_twiddle) table_get(w, table, (size_t)ti << tshift);
    if (DIT) {
        if (has_twiddle) fr::mont_mul(b, b, w);
        fr::sub(d, a, b);
        fr::add(a, a, b);
#pragma unroll
        for (int k = 0; k < NW; k++) b[k] = d[k];
    } else {
        fr::sub(d, a, b);
        fr::add(a, a, b);
        if (has_twiddle) fr::mont_mul(b, d, w);
        else {
#pragma unroll
            for (int k = 0; k < NW; k++) b[k] = d[k];
        }
    }
}

// One workgroup per blob.  zc[j][d], d < M: the coefficients of Z_j, canonical; all zero when fewer than M / 2 cells are present.
// Lane t holds the coefficients t, t + 256 and t + 512 of a step: the degree never exceeds M / 2 <= 512.
__global__ __launch_bounds__(TPB) void k_rec_vanish(const uint8_t* __restrict__ present, const uint32_t* __restrict__ table, uint32_t tshift_m, uint32_t mu,
                                                    uint32_t bitrev, uint64_t* zc, int32_t* ok) {
    __shared__ uint32_t z[NW * TILE];
    __shared__ uint32_t pres[TILE];
    const uint32_t q = threadIdx.x, j = blockIdx.x, M = 1u << mu;
    for (uint32_t m = q; m < M; m += TPB) pres[m] = present[((size_t)j << mu) + m] ? 1u : 0u;
    for (uint32_t d = q; d < TILE; d += TPB) {
#pragma unroll
        for (int k = 0; k < NW; k++) z[k * TILE + d] = (d == 0 && k == 0) ? 1u : 0u;
    }
    __syncthreads();
    uint32_t have = 0;
    for (uint32_t m = 0; m < M; m++) have += pres[m];
    const bool enough = 2 * have >= M;
    if (enough) {
        uint32_t deg = 0;
#pragma unroll 1
        for (uint32_t m = 0; m < M; m++) {
            if (pres[m]) continue;                                  // uniform over the workgroup
            const uint32_t mp = bitrev ? poly::bitrev(m, mu) : m;
            uint32_t w[NW], v[3][NW];
            table_get(w, table, (size_t)mp << tshift_m);
            // Z <- Z (Y - w): new[d] = old[d - 1] - w old[d], d <= deg + 1 (old[deg + 1] is zero)
#pragma unroll
            for (uint32_t r = 0; r < 3; r++) {
                const uint32_t d = q + r * TPB;
                if (d > deg + 1) continue;
                uint32_t lo[NW];
#pragma unroll
                for (int k = 0; k < NW; k++) {
                    v[r][k] = z[k * TILE + d];
                    lo[k] = d ? z[k * TILE + d - 1] : 0u;
                }
                fr::mont_mul(v[r], v[r], w);
                fr::sub(v[r], lo, v[r]);
            }
            __syncthreads();
#pragma unroll
            for (uint32_t r = 0; r < 3; r++) {
                const uint32_t d = q + r * TPB;
                if (d > deg + 1) continue;
#pragma unroll
                for (int k = 0; k < NW; k++) z[k * TILE + d] = v[r][k];
            }
            __syncthreads();
            deg++;
        }
    }
    for (uint32_t d = q; d < M; d += TPB) {
        uint32_t v[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) v[k] = enough ? z[k * TILE + d] : 0u;
        fr::wire_store(zc + 4 * (((size_t)j << mu) + d), v);
    }
    if (q == 0) ok[j] = enough ? 1 : 0;
}

// the inclusive prefix products (Montgomery products: canonical elements taken as Montgomery forms) of sh[0 .. M), in place
__device__ __forceinline__ void product_scan(uint32_t* sh, uint32_t M, uint32_t q) {
#pragma unroll 1
    for (uint32_t d = 1; d < M; d <<= 1) {
        uint32_t v[4][NW];
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint32_t t = q + r * TPB;
            if (t >= M || t < d) continue;
            uint32_t b[NW];
#pragma unroll
            for (int k = 0; k < NW; k++) {
                v[r][k] = sh[k * TILE + t];
                b[k] = sh[k * TILE + t - d];
            }
            fr::mont_mul(v[r], v[r], b);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint32_t t = q + r * TPB;
            if (t >= M || t < d) continue;
#pragma unroll
            for (int k = 0; k < NW; k++) sh[k * TILE + t] = v[r][k];
        }
        __syncthreads();
    }
}

// One workgroup per blob: zs[j][t] <- 1 / zs[j][t] for zs[j][t] = Z_j(7 w_M^t), t < M, by Montgomery's trick with a KNOWN total:
// prod_t Z(7 w_M^t) = c^deg Z, c = 1 - 7^M.  cinv: the Montgomery form of 1 / c; rpow: R^(M - 1) as an integer.  With the exclusive
// prefix E_t and suffix S_t as Montgomery products (E_0 = S_{M-1} = one), E_t S_t = prod_{s != t} zs[s] / R^(M-2), and the Montgomery
// product with W = c^-deg R^(M-1) is the canonical inverse.  A blob with too few cells keeps its zero table.
__global__ __launch_bounds__(TPB) void k_rec_zinv(const uint8_t* __restrict__ present, uint32_t mu, FrWords cinv, FrWords rpow, uint64_t* zs) {
    constexpr fr::Consts K = fr::make_consts();
    __shared__ uint32_t sh[NW * TILE];
    __shared__ uint32_t pres[TILE];
    const uint32_t q = threadIdx.x, j = blockIdx.x, M = 1u << mu;
    uint64_t* row = zs + 4 * ((size_t)j << mu);
    for (uint32_t m = q; m < M; m += TPB) pres[m] = present[((size_t)j << mu) + m] ? 1u : 0u;
    __syncthreads();
    uint32_t have = 0;
    for (uint32_t m = 0; m < M; m++) have += pres[m];
    if (2 * have < M) return;                                       // uniform over the workgroup
    uint32_t wv[NW], base[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) {
        wv[k] = rpow.w[k];
        base[k] = cinv.w[k];
    }
#pragma unroll 1
    for (uint32_t e = M - have; e; e >>= 1) {
        if (e & 1) fr::mont_mul(wv, wv, base);
        fr::mont_mul(base, base, base);
    }
    uint32_t ex[4][NW];
#pragma unroll 1
    for (uint32_t side = 0; side < 2; side++) {                     // 0: prefixes of the row, 1: of the row reversed - the suffixes
        for (uint32_t t = q; t < M; t += TPB) {
            uint32_t v[NW];
            fr::wire_load(v, row + 4 * (size_t)(side ? M - 1 - t : t));
#pragma unroll
            for (int k = 0; k < NW; k++) sh[k * TILE + t] = v[k];
        }
        __syncthreads();
        product_scan(sh, M, q);
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint32_t t = q + r * TPB;
            if (t >= M) continue;
            // side 0: the product of the entries before t; side 1: of the entries behind it, M - 1 - t of them
            const uint32_t cnt = side ? M - 1 - t : t;
            uint32_t v[NW];
#pragma unroll
            for (int k = 0; k < NW; k++) v[k] = cnt ? sh[k * TILE + cnt - 1] : K.one[k];
            if (side) fr::mont_mul(ex[r], ex[r], v);
            else {
#pragma unroll
                for (int k = 0; k < NW; k++) ex[r][k] = v[k];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) {
        const uint32_t t = q + r * TPB;
        if (t >= M) continue;
        fr::mont_mul(ex[r], ex[r], wv);
        fr::wire_store(row + 4 * (size_t)t, ex[r]);
    }
}

// the constants of k_rec_zinv for M = 2^mu, computed once: 1 / (1 - 7^M) in Montgomery form and R^(M-1) as an integer
struct ZinvConsts { FrWords cinv[poly::TILE_LOG2 + 1], rpow[poly::TILE_LOG2 + 1]; };
inline const ZinvConsts& zinv_consts() {
    static const ZinvConsts T = [] {
        constexpr fr::Consts K = fr::make_consts();
        ZinvConsts t{};
        for (unsigned mu = 1; mu <= poly::TILE_LOG2; mu++) {
            const uint32_t seven[NW] = {7, 0, 0, 0, 0, 0, 0, 0};
            uint32_t x[NW], c[NW], p[NW], b[NW];
            fr::to_mont(x, seven);
            for (unsigned i = 0; i < mu; i++) fr::mont_mul(x, x, x);
            fr::sub(c, K.one, x);
            fr::mont_inv(t.cinv[mu].w, c);
            for (int k = 0; k < NW; k++) {      // the Montgomery form of R is R^2: its power M - 2 is R^(M-1) as an integer
                p[k] = K.one[k];
                b[k] = K.r2[k];
            }
            for (uint32_t e = (1u << mu) - 2; e; e >>= 1) {
                if (e & 1) fr::mont_mul(p, p, b);
                fr::mont_mul(b, b, b);
            }
            for (int k = 0; k < NW; k++) t.rpow[mu].w[k] = p[k];
        }
        return t;
    }();
    return T;
}

// the mu stages over the position bits of the tile, in place: decimation in frequency (natural order in, position s holds entry
// bitrev(s) after) or in time (the reverse); unscaled
template <bool DIT>
__device__ __forceinline__ void column_transform(uint32_t* sh, const uint32_t* __restrict__ table, const rec::Column& a, uint32_t inverse, uint32_t q) {
    const poly::Pass P = rec::pass_of(a.mu, a.cl, DIT ? 1u : 0u);
    const uint32_t rounds = poly::n_rounds(P);
#pragma unroll 1
    for (uint32_t r = 0; r < rounds; r++) {
        const poly::Round R = poly::round_of(P, r);
        const uint32_t e0 = poly::round_element(R, q, 0), e1 = poly::round_element(R, q, 1), e2 = poly::round_element(R, q, 2),
                       e3 = poly::round_element(R, q, 3);
        uint32_t x0[NW], x1[NW], x2[NW], x3[NW];
        tile_get(x0, sh, e0);
        tile_get(x1, sh, e1);
        tile_get(x2, sh, e2);
        tile_get(x3, sh, e3);
        const bool tw_lo = R.pos != a.cl;      // the stage on position bit 0 has twiddle one throughout
        if (DIT) {
            if (R.lo) {
                const uint32_t ti = rec::twiddle_exp(a.mu, a.cl, e0, R.pos, inverse);
                butterfly<true>(x0, x1, table, a.tshift_m, ti, tw_lo);
                butterfly<true>(x2, x3, table, a.tshift_m, ti, tw_lo);
            }
            if (R.hi) {
                butterfly<true>(x0, x2, table, a.tshift_m, rec::twiddle_exp(a.mu, a.cl, e0, R.pos + 1, inverse), true);
                butterfly<true>(x1, x3, table, a.tshift_m, rec::twiddle_exp(a.mu, a.cl, e1, R.pos + 1, inverse), true);
            }
        } else {
            if (R.hi) {
                butterfly<false>(x0, x2, table, a.tshift_m, rec::twiddle_exp(a.mu, a.cl, e0, R.pos + 1, inverse), true);
                butterfly<false>(x1, x3, table, a.tshift_m, rec::twiddle_exp(a.mu, a.cl, e1, R.pos + 1, inverse), true);
            }
            if (R.lo) {
                const uint32_t ti = rec::twiddle_exp(a.mu, a.cl, e0, R.pos, inverse);
                butterfly<false>(x0, x1, table, a.tshift_m, ti, tw_lo);
                butterfly<false>(x2, x3, table, a.tshift_m, ti, tw_lo);
            }
        }
        tile_put(sh, e0, x0);
        tile_put(sh, e1, x1);
        tile_put(sh, e2, x2);
        tile_put(sh, e3, x3);
        __syncthreads();
    }
}

// Workgroup (j, g): columns g C .. g C + C - 1 of blob j.  Tile element e = c | (p << cl): column slot c, position p.
__global__ __launch_bounds__(TPB) void k_rec_column(const uint64_t* __restrict__ coef, const uint8_t* __restrict__ present, const uint64_t* __restrict__ zr,
                                                    const uint64_t* __restrict__ zsinv, const uint32_t* __restrict__ table,
                                                    const uint32_t* __restrict__ coset, rec::Column a, FrWords scale, uint64_t* out, int32_t* ok) {
    __shared__ uint32_t sh[NW * TILE];
    const uint32_t q = threadIdx.x;
    const uint32_t j = blockIdx.x / a.groups, i0 = (blockIdx.x % a.groups) * a.cols;
    const uint32_t cmask = poly::low_mask(a.cl);
    const size_t cell0 = (size_t)j << a.mu;
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t e = u * TPB + q, c = e & cmask, p = e >> a.cl;
        uint32_t v[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) v[k] = 0;
        if (c < a.cols) {
            const uint32_t m = a.bitrev ? poly::bitrev(p, a.mu) : p;
            if (present[cell0 + m]) {
                const uint32_t i = i0 + c;
                uint32_t w[NW];
                fr::wire_load(v, coef + 4 * (((cell0 + m) << a.log2_l) + i));
                table_get(w, table, (size_t)rec::inverse_power(p, i, a.log2_d) << a.tshift_d);
                fr::mont_mul(v, v, w);                              // coefficient i of the interpolant on the coset: canonical
                fr::wire_load(w, zr + 4 * (cell0 + p));
                fr::mont_mul(v, v, w);                              // E Z / R
            }
        }
        tile_put(sh, e, v);
    }
    __syncthreads();
    column_transform<false>(sh, table, a, 1, q);                    // position s: M q_{bitrev(s)}
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t e = u * TPB + q;
        if ((e & cmask) >= a.cols) continue;
        uint32_t v[NW];
        tile_get(v, sh, e);
        coset_mul(v, coset, poly::bitrev(e >> a.cl, a.mu), 0);
        tile_put(sh, e, v);
    }
    __syncthreads();
    column_transform<true>(sh, table, a, 0, q);                     // position t: M q(7 w_M^t)
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t e = u * TPB + q;
        if ((e & cmask) >= a.cols) continue;
        uint32_t v[NW], w[NW];
        tile_get(v, sh, e);
        fr::wire_load(w, zsinv + 4 * (cell0 + (e >> a.cl)));
        fr::mont_mul(v, v, w);
        tile_put(sh, e, v);
    }
    __syncthreads();
    column_transform<false>(sh, table, a, 1, q);                    // position s: M^2 R^-2 7^t p_t, t = bitrev(s)
    const uint32_t half = 1u << (a.mu - 1), log2_n = a.log2_d - 1;
    uint32_t nz = 0;
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t e = u * TPB + q, c = e & cmask;
        if (c >= a.cols) continue;
        const uint32_t t = poly::bitrev(e >> a.cl, a.mu);
        uint32_t v[NW];
        tile_get(v, sh, e);
        if (t < half) {
            fr::mont_mul(v, v, scale.w);
            coset_mul(v, coset, t, 1);
            fr::wire_store(out + 4 * (((size_t)j << log2_n) + ((size_t)t << a.log2_l) + i0 + c), v);
        } else {
#pragma unroll
            for (int k = 0; k < NW; k++) nz |= v[k];
        }
    }
    if (nz) ok[j] = 0;      // every writer stores the same value
}

#ifndef ZKP_RECOVER_KERNELS_ONLY
// validation mode: the values of present cells only
__global__ void k_rec_valid(const uint64_t* __restrict__ values, const uint8_t* __restrict__ present, size_t n_el, uint32_t log2_l, int* bad) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_el || !present[id >> log2_l]) return;
    uint32_t v[NW];
    fr::wire_load(v, values + 4 * id);
    if (!fr::is_canonical(v)) atomicOr(bad, 1);
}
#endif

}  // namespace

#ifndef ZKP_RECOVER_KERNELS_ONLY
#define REC_CHK(c, what, call)                                       \
    do {                                                             \
        if (int rc__ = ctxop::fail((c), (what), (call))) return rc__; \
    } while (0)

hipError_t rec_check_present(const uint64_t* values, const uint8_t* present, size_t rows, unsigned log2_l, int* bad, hipStream_t s) {
    const size_t n_el = rows << log2_l;
    if (!n_el) return hipSuccess;
    hipLaunchKernelGGL(k_rec_valid, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, s, values, present, n_el, (uint32_t)log2_l, bad);
    return hipGetLastError();
}

int recover_dev(zkp_ctx* c, const uint64_t* values, const uint8_t* present, size_t n, unsigned log2_n, unsigned log2_l, int flags, uint64_t* out_coeffs,
                int32_t* out_ok, hipStream_t s) {
    if (!n) return 0;
    constexpr fr::Roots ROOTS = fr::make_roots();
    constexpr fr::Consts K = fr::make_consts();
    const rec::Shape sh = rec::shape_of(log2_n, log2_l);
    const rec::Layout L = rec::layout(n, log2_n, log2_l, flags);
    // the workspace and the tables first (an allocation synchronises the device), then only launches
    void* ws = nullptr;
    const uint32_t *table = nullptr, *coset = nullptr;
    unsigned table_log2 = 0;
    int rc;
    if ((rc = ctxop::grow_kzg(c, L.total, &ws)) || (rc = ctxop::kzg_domain(c, sh.log2_d, &table, &table_log2, s)) || (rc = ctxop::poly_coset(c, &coset, s))) return rc;
    char* w = (char*)ws;
    uint64_t *coef = (uint64_t*)(w + L.coef), *zc = (uint64_t*)(w + L.zc), *zr = (uint64_t*)(w + L.zr), *zs = (uint64_t*)(w + L.zs);
    const rec::Column a = rec::column_of(log2_n, log2_l, flags, table_log2);
    FrWords scale;      // 2^-2mu R^3 as an integer: the Montgomery product with it multiplies by 2^-2mu R^2
    fr::mont_mul(scale.w, ROOTS.inv_pow2[2 * sh.mu], K.r2);
    fr::mont_mul(scale.w, scale.w, K.r2);
    const int nflags = poly::NTT_INVERSE | (flags & poly::NTT_BITREV);
    const ZinvConsts& zc_consts = zinv_consts();
    for (size_t at = 0; at < n; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        const uint64_t* v = values + 4 * (at << sh.log2_d);
        const uint8_t* pr = present + (at << sh.mu);
        const uint64_t* cf = v;
        if (log2_l) {
            REC_CHK(c, "fr_ntt", fr_ntt(w + L.ntt, table, table_log2, nullptr, v, cnt << sh.mu, log2_l, nflags, coef, s));
            cf = coef;
        }
        hipLaunchKernelGGL(k_rec_vanish, dim3((unsigned)cnt), dim3(TPB), 0, s, pr, table, a.tshift_m, a.mu, a.bitrev, zc, out_ok + at);
        REC_CHK(c, "k_rec_vanish", hipGetLastError());
        REC_CHK(c, "fr_ntt", fr_ntt(nullptr, table, table_log2, nullptr, zc, cnt, sh.mu, 0, zr, s));
        REC_CHK(c, "fr_ntt", fr_ntt(nullptr, table, table_log2, coset, zc, cnt, sh.mu, poly::NTT_COSET, zs, s));
        hipLaunchKernelGGL(k_rec_zinv, dim3((unsigned)cnt), dim3(TPB), 0, s, pr, a.mu, zc_consts.cinv[a.mu], zc_consts.rpow[a.mu], zs);
        REC_CHK(c, "k_rec_zinv", hipGetLastError());
        hipLaunchKernelGGL(k_rec_column, dim3((unsigned)(cnt * sh.groups)), dim3(TPB), 0, s, cf, pr, (const uint64_t*)zr, (const uint64_t*)zs, table, coset, a, scale,
                           out_coeffs + 4 * (at << log2_n), out_ok + at);
        REC_CHK(c, "k_rec_column", hipGetLastError());
    }
    return 0;
}
#endif

}  // namespace zkp
