// zkp_fk20.hip -- the batched G1 NTT (zkp_g1_ntt_batch) and the FK20 proofs of a polynomial at every domain point (zkp_kzg_fk20_setup,
// zkp_kzg_fk20_batch).  The group kernels live in zkp_coop.hip beside the group law they use (k_g1ntt_first, k_g1ntt_stage, k_g1ntt_out,
// k_fk20_mul); this file holds the two Fr kernels and the launch sequences.  Every index, grid and byte count: zkp_fk20_plan.hpp.
//
// G1 NTT of a slice: first (bit 0, reads the wire) - one twiddled stage per further bit - out (one inversion per point, the inverse's
// [N^-1]).  k + 1 launches for N = 2^k; a stage is one 128-doubling scalar multiplication and two full additions per butterfly.
//
// FK20 of a slice of polynomials, N = 2^k:
//   1. k_fk20_coeffs   c = (f_{N-1}, 0 x (N + 1), f_1 .. f_{N-2}) / (2 N), one Montgomery product per non-zero entry
//   2. fr_ntt          size 2 N, forward, bit-reversed evaluations, in place
//   3. k_fk20_mul      record t <- [c^[t]] setup[bitrev(t)]: the 2 N products, left Jacobian, in the order the decimation in time reads
//   4. the inverse G1 transform of size 2 N in place, unscaled (step 1 paid for it): h is its first N records, record N - 1 the identity
//   5. the forward G1 transform of size N of h: its first stage reads the lower half of each 2 N block bit-reversed and writes the upper
//      half, which nobody needs any more; the stages run there; out stores the proofs in the order asked for
#include "zkp_fk20.hpp"

#include "zkp_coop.hpp"
#include "zkp_fr.hpp"

namespace zkp {
namespace {

using fr::NW;
constexpr fr::Roots ROOTS = fr::make_roots();
struct FrWords { uint32_t w[NW]; };

// c[j][i] of polynomial j, i < 2 N, scaled by ninv = (2 N)^-1 (Montgomery form: the product is canonical)
__global__ __launch_bounds__(256) void k_fk20_coeffs(const uint64_t* __restrict__ coeffs, uint64_t* c, uint32_t n_el, uint32_t k, FrWords ninv) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_el) return;
    const uint32_t j = t >> (k + 1), i = t & fk20::low_mask(k + 1);
    const int64_t src = fk20::coeff_source(i, k);
    uint32_t v[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) v[w] = 0;
    if (src >= 0) {
        fr::wire_load(v, coeffs + 4 * (((size_t)j << k) + (size_t)src));
        fr::mont_mul(v, v, ninv.w);
    }
    fr::wire_store(c + 4 * (size_t)t, v);
}

// split[i] = (a, b) with domain[i] = a + b z^2 mod r; the domain table is in Montgomery form
__global__ __launch_bounds__(256) void k_g1ntt_split(const uint32_t* __restrict__ domain, uint32_t n, uint64_t* split) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t m[NW], s[NW], a[4], b[4];
#pragma unroll
    for (int w = 0; w < NW; w++) m[w] = domain[(size_t)i * NW + w];
    fr::from_mont(s, m);
    fk20::split_z2(s, a, b);
    split[4 * (size_t)i] = (uint64_t)a[0] | ((uint64_t)a[1] << 32);
    split[4 * (size_t)i + 1] = (uint64_t)a[2] | ((uint64_t)a[3] << 32);
    split[4 * (size_t)i + 2] = (uint64_t)b[0] | ((uint64_t)b[1] << 32);
    split[4 * (size_t)i + 3] = (uint64_t)b[2] | ((uint64_t)b[3] << 32);
}

#define FK_CHK(c, what, call)                                        \
    do {                                                             \
        if (int rc__ = ctxop::fail((c), (what), (call))) return rc__; \
    } while (0)

}  // namespace

// the twiddled stages 1 .. k - 1 of the transforms of `at`
int run_stages(zkp_ctx* c, void* rec, const uint64_t* split, unsigned table_log2, const fk20::Span& at, bool inverse, hipStream_t s) {
    for (uint32_t p = 1; p < at.k; p++) {
        fk20::Stage st;
        st.at = at;
        st.p = p;
        st.inverse = inverse;
        st.tshift = table_log2 - at.k;
        st.n_bfly = at.n_vec << (at.k - 1);
        FK_CHK(c, "k_g1ntt_stage", g1ntt_stage(rec, split, st, s));
    }
    return 0;
}
fk20::First first_of(const fk20::Span& at, uint32_t mode, bool perm, uint32_t src_off) {
    fk20::First f;
    f.at = at;
    f.mode = mode;
    f.perm = perm;
    f.src_off = src_off;
    f.n_lane = at.k ? at.n_vec << (at.k - 1) : at.n_vec;
    return f;
}
fk20::Out out_of(const fk20::Span& at, bool perm, bool scale) {
    fk20::Out o;
    o.at = at;
    o.perm = perm;
    o.scale = scale;
    o.n_pt = at.n_vec << at.k;
    return o;
}
namespace {
// (a_lo, a_hi, b_lo, b_hi) of 2^-k mod r
void split_of_inverse(unsigned k, uint64_t* ab) {
    uint32_t s[NW], a[4], b[4];
    fr::from_mont(s, ROOTS.inv_pow2[k]);
    fk20::split_z2(s, a, b);
    ab[0] = (uint64_t)a[0] | ((uint64_t)a[1] << 32);
    ab[1] = (uint64_t)a[2] | ((uint64_t)a[3] << 32);
    ab[2] = (uint64_t)b[0] | ((uint64_t)b[1] << 32);
    ab[3] = (uint64_t)b[2] | ((uint64_t)b[3] << 32);
}

}  // namespace

hipError_t g1ntt_split_build(const uint32_t* domain, unsigned log2_n, uint64_t* split, hipStream_t s) {
    const uint32_t n = 1u << log2_n;
    hipLaunchKernelGGL(k_g1ntt_split, dim3((n + 255) / 256), dim3(256), 0, s, domain, n, split);
    return hipGetLastError();
}

int g1_ntt_dev(zkp_ctx* c, const uint64_t* points, const uint8_t* inf, size_t n_vec, unsigned log2_n, int flags, uint64_t* out, uint8_t* out_inf, hipStream_t s) {
    if (!n_vec) return 0;
    const size_t slice = fk20::slice_vectors(n_vec, log2_n);
    void* rec = nullptr;
    const uint32_t* domain = nullptr;
    const uint64_t* split = nullptr;
    unsigned table_log2 = 0;
    int rc;
    // the workspaces first (an allocation synchronises the device), then only launches
    if ((rc = ctxop::grow_fk20(c, fk20::g1ntt_workspace_bytes(n_vec, log2_n), &rec)) || (rc = ctxop::g1ntt_tables(c, log2_n, &domain, &split, &table_log2, s)))
        return rc;
    const bool inverse = flags & fk20::NTT_INVERSE, brv = flags & fk20::NTT_BITREV;
    uint64_t ab[4] = {0, 0, 0, 0};
    if (inverse) split_of_inverse(log2_n, ab);
    for (size_t at = 0; at < n_vec; at += slice) {
        const size_t cnt = n_vec - at < slice ? n_vec - at : slice;
        fk20::Span sp;
        sp.k = log2_n;
        sp.vs_log2 = log2_n;
        sp.n_vec = (uint32_t)cnt;
        FK_CHK(c, "k_g1ntt_first", g1ntt_first(points + 12 * (at << log2_n), inf ? inf + (at << log2_n) : nullptr, rec,
                                               first_of(sp, fk20::SRC_WIRE, !(inverse && brv), 0), s));
        if ((rc = run_stages(c, rec, split, table_log2, sp, inverse, s))) return rc;
        FK_CHK(c, "k_g1ntt_out", g1ntt_out(rec, out + 12 * (at << log2_n), out_inf + (at << log2_n), out_of(sp, !inverse && brv, inverse && log2_n), ab, s));
    }
    return 0;
}

int fk20_setup_dev(zkp_ctx* c, const uint64_t* monomial, unsigned log2_n, uint64_t* out, uint8_t* out_inf, hipStream_t s) {
    const unsigned k1 = log2_n + 1;
    void* rec = nullptr;
    const uint32_t* domain = nullptr;
    const uint64_t* split = nullptr;
    unsigned table_log2 = 0;
    int rc;
    if ((rc = ctxop::grow_fk20(c, fk20::g1ntt_workspace_bytes(1, k1), &rec)) || (rc = ctxop::g1ntt_tables(c, k1, &domain, &split, &table_log2, s))) return rc;
    const uint64_t ab[4] = {0, 0, 0, 0};
    fk20::Span sp;
    sp.k = k1;
    sp.vs_log2 = k1;
    sp.n_vec = 1;
    FK_CHK(c, "k_g1ntt_first", g1ntt_first(monomial, nullptr, rec, first_of(sp, fk20::SRC_SETUP, true, 0), s));
    if ((rc = run_stages(c, rec, split, table_log2, sp, false, s))) return rc;
    FK_CHK(c, "k_g1ntt_out", g1ntt_out(rec, out, out_inf, out_of(sp, false, false), ab, s));
    return 0;
}

int fk20_dev(zkp_ctx* c, const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* coeffs, size_t n, unsigned log2_n, int flags, uint64_t* out_proof,
             uint8_t* out_inf, hipStream_t s) {
    if (!n) return 0;
    const unsigned k = log2_n, k1 = log2_n + 1;
    const fk20::Fk20Layout L = fk20::fk20_layout(n, k);
    void* ws = nullptr;
    const uint32_t* domain = nullptr;
    const uint64_t* split = nullptr;
    unsigned table_log2 = 0;
    int rc;
    if ((rc = ctxop::grow_fk20(c, L.total, &ws)) || (rc = ctxop::g1ntt_tables(c, k1, &domain, &split, &table_log2, s))) return rc;
    void* rec = (char*)ws + L.rec;
    uint64_t* cf = (uint64_t*)((char*)ws + L.fr);
    FrWords ninv;
    for (int w = 0; w < NW; w++) ninv.w[w] = ROOTS.inv_pow2[k1][w];
    const uint64_t ab[4] = {0, 0, 0, 0};
    for (size_t at = 0; at < n; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        const uint32_t pts = (uint32_t)(cnt << k1);
        hipLaunchKernelGGL(k_fk20_coeffs, dim3((pts + 255) / 256), dim3(256), 0, s, coeffs + 4 * (at << k), cf, pts, (uint32_t)k, ninv);
        FK_CHK(c, "k_fk20_coeffs", hipGetLastError());
        FK_CHK(c, "fr_ntt", fr_ntt(nullptr, domain, table_log2, nullptr, cf, cnt, k1, fk20::NTT_BITREV, cf, s));
        FK_CHK(c, "k_fk20_mul", fk20_mul(setup, setup_inf, cf, pts, k1, rec, s));
        fk20::Span big;       // the inverse transform of size 2 N, in place, input already in the decimation's order
        big.k = k1;
        big.vs_log2 = k1;
        big.n_vec = (uint32_t)cnt;
        FK_CHK(c, "k_g1ntt_first", g1ntt_first(nullptr, nullptr, rec, first_of(big, fk20::SRC_REC, false, 0), s));
        if ((rc = run_stages(c, rec, split, table_log2, big, true, s))) return rc;
        fk20::Span low;       // the forward transform of size N of h: from the lower half of a block into its upper half
        low.k = k;
        low.vs_log2 = k1;
        low.off = 1u << k;
        low.n_vec = (uint32_t)cnt;
        FK_CHK(c, "k_g1ntt_first", g1ntt_first(nullptr, nullptr, rec, first_of(low, fk20::SRC_REC, true, 0), s));
        if ((rc = run_stages(c, rec, split, table_log2, low, false, s))) return rc;
        FK_CHK(c, "k_g1ntt_out", g1ntt_out(rec, out_proof + 12 * (at << k), out_inf + (at << k), out_of(low, flags & fk20::NTT_BITREV, false), ab, s));
    }
    return 0;
}

}  // namespace zkp
