// zkp_cells.hip -- the KZG cell proofs: FK20 multi-proofs, one per coset of l points (zkp_kzg_cells_setup, zkp_kzg_cells_batch).  The group
// kernels live in zkp_coop.hip beside the group law they use (k_cell_mac, k_cell_sum, and the transforms' k_g1ntt_*); this file holds the
// Fr kernel and the launch sequences.  Every index, grid and byte count: zkp_cells_plan.hpp and zkp_fk20_plan.hpp.
//
// A slice of polynomials, N = l k, M = e k proofs each, a block of 2 M records per polynomial:
//   1. k_cell_coeffs   c_i = (f_{N-1-i}, 0 x (k + 1), f_{2l-1-i}, .., f_{N-l-1-i}) / (2 k) for every stride i < l
//   2. fr_ntt          size 2 k over the l vectors of every polynomial, forward, bit-reversed evaluations, in place
//   3. k_cell_mac      a partial per (slot, group of g strides): sum over the group of [c^_i[t]] X_i[bitrev(t)], one chain of doublings
//      k_cell_sum      record t of the block <- the sum of the slot's l / g partials (not launched when g = l: the chain wrote the record)
//   4. the inverse G1 transform of size 2 k in the first 2 k records of the block, unscaled: h is its first k records
//   5. the forward G1 transform of size M of (h, identities): its first stage reads the first k records bit-reversed - an input from k on
//      IS the identity, whatever its record holds - and writes the upper half of the block; out stores the proofs in the order asked for
#include "zkp_cells.hpp"

#include "zkp_coop.hpp"
#include "zkp_fr.hpp"
#include "zkp_groth16_plan.hpp"
#include "zkp_msm.hpp"
#include "zkp_msm_plan.hpp"
#include "zkp_poly_plan.hpp"
#include "zkp_rlc_plan.hpp"

namespace zkp {
namespace {

using fr::NW;
constexpr fr::Roots ROOTS = fr::make_roots();
struct FrWords { uint32_t w[NW]; };

// element t of vector i of polynomial j, scaled by ninv = (2 k)^-1 (Montgomery form: the product is canonical)
__global__ __launch_bounds__(256) void k_cell_coeffs(const uint64_t* __restrict__ coeffs, uint64_t* c, uint32_t n_el, uint32_t log2_n, uint32_t log2_l, FrWords ninv) {
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    if (id >= n_el) return;
    const uint32_t k1 = log2_n - log2_l + 1;
    const uint32_t t = id & fk20::low_mask(k1), i = (id >> k1) & fk20::low_mask(log2_l), j = id >> (k1 + log2_l);
    const int64_t src = cells::coeff_source(t, i, k1 - 1, log2_l);
    uint32_t v[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) v[w] = 0;
    if (src >= 0) {
        fr::wire_load(v, coeffs + 4 * (((size_t)j << log2_n) + (size_t)src));
        fr::mont_mul(v, v, ninv.w);
    }
    fr::wire_store(c + 4 * (size_t)id, v);
}

// ------------------------------------------------------------------------------------------------------------------ the verifier's small kernels
inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }
// Element (j, i) of the coefficients: coef[j][i] <- coef[j][i] c_j^-i with c_j = w_D^m', c_j^-i an entry of the domain table (Montgomery
// form: the product of a canonical element with it is canonical).  The lane of i = 0 also writes row j of the scalars: ms[j] = r_j =
// a_j + b_j z^2 exactly as zkp_pairing_check_batch_rlc forms it, ms[n + j] = r_j c_j^l, row 1 = 0 | r_j.  A value >= r, an index >= M
// and a zero (a, b) clear flag[0]; an index >= M is then read as index mod M, so nothing is read out of bounds.
__global__ __launch_bounds__(256) void k_cell_scale(uint64_t* coef, const uint64_t* __restrict__ values, const uint32_t* __restrict__ index,
                                                    const uint64_t* __restrict__ rand, const uint32_t* __restrict__ table, uint32_t tshift, uint32_t n,
                                                    uint32_t log2_d, uint32_t log2_l, uint32_t bitrev, uint32_t terms, uint64_t* ms, int* flag) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= ((size_t)n << log2_l)) return;
    const uint32_t j = (uint32_t)(id >> log2_l), i = (uint32_t)id & fk20::low_mask(log2_l), log2_m = log2_d - log2_l;
    const uint32_t raw = index[j], m = raw & fk20::low_mask(log2_m), mp = bitrev ? fk20::bitrev(m, log2_m) : m;
    uint32_t v[NW], w[NW];
    fr::wire_load(v, values + 4 * id);
    if (!fr::is_canonical(v) || raw != m) flag[0] = 0;
    fr::wire_load(v, coef + 4 * id);
    const uint32_t e = cells::inverse_power_index(mp, i, log2_d) << tshift;
#pragma unroll
    for (int k = 0; k < NW; k++) w[k] = table[(size_t)e * NW + k];
    fr::mont_mul(v, v, w);
    fr::wire_store(coef + 4 * id, v);
    if (i) return;
    const uint64_t a = rand[2 * (size_t)j], b = rand[2 * (size_t)j + 1];
    uint64_t r[rlc::SCALAR_U64];
    rlc::scalar(a, b, r);
    if (!a && !b) flag[0] = 0;
    uint32_t rw[NW];
    fr::wire_load(rw, r);
    const uint32_t el = (uint32_t)(((uint64_t)mp << log2_l) & fk20::low_mask(log2_d)) << tshift;      // c_j^l = w_D^(m' l)
#pragma unroll
    for (int k = 0; k < NW; k++) w[k] = table[(size_t)el * NW + k];
    fr::mont_mul(rw, rw, w);
    uint64_t* row1 = ms + 4 * (size_t)terms;
    for (size_t k = 0; k < rlc::SCALAR_U64; k++) {
        ms[4 * (size_t)j + k] = r[k];
        row1[4 * (size_t)j + k] = 0;
        row1[4 * ((size_t)n + j) + k] = r[k];
    }
    fr::wire_store(ms + 4 * ((size_t)n + j), rw);
}
// The MSM's operands: points C | pi | monomial with their infinity bytes; behind the scalars r | r c^l of row 0 the l scalars -a_i, and
// zeros behind row 1
__global__ void k_cell_place(const uint64_t* cp, const uint8_t* cinf, const uint64_t* pp, const uint8_t* pinf, const uint64_t* mono, const uint64_t* a, size_t n,
                             size_t l, uint64_t* mp, uint8_t* minf, uint64_t* ms) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, terms = 2 * n + l;
    if (i < 12 * n) mp[i] = cp[i];
    else if (i < 24 * n) mp[i] = pp[i - 12 * n];
    else if (i < 12 * terms) mp[i] = mono[i - 24 * n];
    if (i < n) minf[i] = cinf ? cinf[i] : 0;
    else if (i < 2 * n) minf[i] = pinf ? pinf[i - n] : 0;
    else if (i < terms) minf[i] = 0;
    if (i < l) {
        uint32_t aw[NW];
        fr::wire_load(aw, a + 4 * i);
        fr::neg(aw, aw);
        fr::wire_store(ms + 4 * (2 * n + i), aw);
        for (int w = 0; w < 4; w++) ms[4 * (terms + 2 * n + i) + w] = 0;
    }
}

#define CL_CHK(c, what, call)                                        \
    do {                                                             \
        if (int rc__ = ctxop::fail((c), (what), (call))) return rc__; \
    } while (0)

}  // namespace

int cells_setup_dev(zkp_ctx* c, const uint64_t* monomial, unsigned log2_n, unsigned log2_l, uint64_t* out, uint8_t* out_inf, hipStream_t s) {
    const cells::Shape sh = cells::shape_of(log2_n, log2_l, 0);
    void* rec = nullptr;
    const uint32_t* domain = nullptr;
    const uint64_t* split = nullptr;
    unsigned table_log2 = 0;
    int rc;
    if ((rc = ctxop::grow_fk20(c, cells::setup_workspace_bytes(log2_n), &rec)) || (rc = ctxop::g1ntt_tables(c, sh.k1, &domain, &split, &table_log2, s))) return rc;
    const uint64_t ab[4] = {0, 0, 0, 0};
    fk20::Span sp;      // l vectors of 2 k points, one after the other: out[i][t]
    sp.k = sh.k1;
    sp.vs_log2 = sh.k1;
    sp.n_vec = 1u << log2_l;
    fk20::First first = first_of(sp, fk20::SRC_CELLS, true, 0);
    first.log2_l = log2_l;
    CL_CHK(c, "k_g1ntt_first", g1ntt_first(monomial, nullptr, rec, first, s));
    if ((rc = run_stages(c, rec, split, table_log2, sp, false, s))) return rc;
    CL_CHK(c, "k_g1ntt_out", g1ntt_out(rec, out, out_inf, out_of(sp, false, false), ab, s));
    return 0;
}

int cells_dev(zkp_ctx* c, const uint64_t* setup, const uint8_t* setup_inf, const uint64_t* coeffs, size_t n, unsigned log2_n, unsigned log2_l, unsigned log2_ext,
              int flags, uint64_t* out_proof, uint8_t* out_inf, hipStream_t s) {
    if (!n) return 0;
    const cells::Shape sh = cells::shape_of(log2_n, log2_l, log2_ext);
    const cells::Layout L = cells::layout(n, log2_n, log2_l, log2_ext);
    void* ws = nullptr;
    const uint32_t* domain = nullptr;
    const uint64_t* split = nullptr;
    unsigned table_log2 = 0;
    int rc;
    if ((rc = ctxop::grow_fk20(c, L.total, &ws)) || (rc = ctxop::g1ntt_tables(c, sh.k1, &domain, &split, &table_log2, s))) return rc;
    void* rec = (char*)ws + L.rec;
    void* part = (char*)ws + L.part;
    uint64_t* cf = (uint64_t*)((char*)ws + L.fr);
    FrWords ninv;
    for (int w = 0; w < NW; w++) ninv.w[w] = ROOTS.inv_pow2[sh.k1][w];
    const uint64_t ab[4] = {0, 0, 0, 0};
    for (size_t at = 0; at < n; at += L.slice) {
        const size_t cnt = n - at < L.slice ? n - at : L.slice;
        const uint32_t els = (uint32_t)(cnt << (log2_n + 1));
        hipLaunchKernelGGL(k_cell_coeffs, dim3((els + 255) / 256), dim3(256), 0, s, coeffs + 4 * (at << log2_n), cf, els, (uint32_t)log2_n, (uint32_t)log2_l, ninv);
        CL_CHK(c, "k_cell_coeffs", hipGetLastError());
        CL_CHK(c, "fr_ntt", fr_ntt(nullptr, domain, table_log2, nullptr, cf, cnt << log2_l, sh.k1, fk20::NTT_BITREV, cf, s));
        cells::Mac mac;
        mac.log2_l = log2_l;
        mac.k1 = sh.k1;
        mac.blk = sh.blk;
        mac.s = L.s;
        mac.n_lane = els >> L.s;
        CL_CHK(c, "k_cell_mac", cell_mac(setup, setup_inf, cf, part, rec, mac, s));
        if (L.s != log2_l) {
            cells::Sum sum;
            sum.log2_l = log2_l;
            sum.k1 = sh.k1;
            sum.blk = sh.blk;
            sum.s = L.s;
            sum.n_lane = (uint32_t)(cnt << sh.k1);
            CL_CHK(c, "k_cell_sum", cell_sum(part, rec, sum, s));
        }
        fk20::Span big;       // the inverse transform of size 2 k in the first 2 k records of a block, input already in the decimation's order
        big.k = sh.k1;
        big.vs_log2 = sh.blk;
        big.n_vec = (uint32_t)cnt;
        CL_CHK(c, "k_g1ntt_first", g1ntt_first(nullptr, nullptr, rec, first_of(big, fk20::SRC_REC, false, 0), s));
        if ((rc = run_stages(c, rec, split, table_log2, big, true, s))) return rc;
        fk20::Span low;       // the forward transform of size M of (h, identities): from the first k records of a block into its upper half
        low.k = sh.m;
        low.vs_log2 = sh.blk;
        low.off = 1u << sh.m;
        low.n_vec = (uint32_t)cnt;
        fk20::First first = first_of(low, fk20::SRC_REC, true, 0);
        first.src_len = 1u << sh.k;
        CL_CHK(c, "k_g1ntt_first", g1ntt_first(nullptr, nullptr, rec, first, s));
        if ((rc = run_stages(c, rec, split, table_log2, low, false, s))) return rc;
        CL_CHK(c, "k_g1ntt_out", g1ntt_out(rec, out_proof + 12 * (at << sh.m), out_inf + (at << sh.m), out_of(low, flags & fk20::NTT_BITREV, false), ab, s));
    }
    return 0;
}

// e(sum r_j C_j + sum r_j c_j^l pi_j - sum_i [a_i] s_i, -g2) * e(sum r_j pi_j, [tau^l]g2) == 1, a_i = sum_j r_j (coefficient i of I_j)
int cell_check_dev(zkp_ctx* c, const CellBatch& b, int flags, int* all_ok, hipStream_t s) {
    const size_t n = b.n, l = (size_t)1 << b.log2_l, terms = 2 * n + l;
    int rc;
    if (!n) {
        return ctxop::fail(c, "k_kzg_init", kzg_flag_init(nullptr, all_ok, 1, s));
    }
    const int nflags = fk20::NTT_INVERSE | (flags & fk20::NTT_BITREV);
    const g16::FoldPlan fp = g16::fold_plan(n, l);
    const cells::VerifyLayout L = cells::verify_layout(n, b.log2_l, flags, poly::ntt_workspace_bytes(n, b.log2_l, nflags), fp.part_bytes);
    // the workspaces and the table first (an allocation synchronises the device), then only launches
    void* ws = nullptr;
    const uint32_t* table = nullptr;
    unsigned table_log2 = 0;
    if ((rc = ctxop::grow_kzg(c, L.total, &ws)) || (rc = ctxop::grow_msm(c, msm_workspace_bytes(1, terms, 2, 1))) ||
        (rc = ctxop::kzg_domain(c, b.log2_d, &table, &table_log2, s)))
        return rc;
    char* w = (char*)ws;
    int* flag = (int*)(w + L.flag);
    uint8_t *st = (uint8_t*)(w + L.st), *minf = (uint8_t*)(w + L.minf), *minf1 = (uint8_t*)(w + L.minf1);
    uint64_t *coef = (uint64_t*)(w + L.coef), *ms = (uint64_t*)(w + L.ms), *mp = (uint64_t*)(w + L.mp), *a = (uint64_t*)(w + L.a);
    uint64_t *mg1 = (uint64_t*)(w + L.mg1), *mg2 = (uint64_t*)(w + L.mg2), *ml = (uint64_t*)(w + L.ml);

    CL_CHK(c, "k_kzg_init", kzg_flag_init(flag, all_ok, 0, s));
    CL_CHK(c, "k_kzg_g2", kzg_g2_side(b.g2, b.tau_l_g2, mg2, s));
    // 1. the interpolants' coefficients on H_l, then on the cosets; the scalars r_j and r_j c_j^l
    CL_CHK(c, "fr_ntt", fr_ntt(w + L.ntt, table, table_log2, nullptr, b.values, n, b.log2_l, nflags, coef, s));
    hipLaunchKernelGGL(k_cell_scale, dim3(blocks(n << b.log2_l)), dim3(256), 0, s, coef, b.values, b.index, b.rand, table, (uint32_t)(table_log2 - b.log2_d),
                       (uint32_t)n, (uint32_t)b.log2_d, (uint32_t)b.log2_l, (uint32_t)((flags & fk20::NTT_BITREV) ? 1 : 0), (uint32_t)terms, ms, flag);
    CL_CHK(c, "k_cell_scale", hipGetLastError());
    // 2. a_i = sum_j r_j coef[j][i]
    CL_CHK(c, "fr_fold", fr_fold(w + L.part, nullptr, ms, coef, n, l, a, nullptr, flag, s));
    // 3. the MSM's points and its last scalars
    hipLaunchKernelGGL(k_cell_place, dim3(blocks(12 * terms)), dim3(256), 0, s, b.c, b.inf_c, b.proof, b.inf_proof, b.monomial, (const uint64_t*)a, n, l, mp, minf,
                       ms);
    CL_CHK(c, "k_cell_place", hipGetLastError());
    // 4. the points check: the statuses side by side, then one fold (-Q is valid exactly when Q is)
    if (L.n_status) {
        uint8_t* at = st;
        auto valid = [&](int which, const void* pts, const void* inf, size_t cnt) -> int {
            const int r = ctxop::valid(c, which, pts, inf, cnt, at, s);
            at += cnt;
            return r;
        };
        if (!(flags & cells::VERIFY_POINTS_CHECKED) && ((rc = valid(1, b.c, b.inf_c, n)) || (rc = valid(1, b.proof, b.inf_proof, n)))) return rc;
        if (!(flags & cells::VERIFY_VK_CHECKED) && ((rc = valid(1, b.monomial, nullptr, l)) || (rc = valid(2, mg2, nullptr, 2)))) return rc;
        CL_CHK(c, "k_kzg_status", kzg_flag_status(st, L.n_status, flag, s));
    }
    // 5. both sums in ONE shared-bases MSM call; 6. the two pairs, one final exponentiation, then the AND
    if ((rc = ctxop::msm_shared(c, 1, mp, minf, ms, terms, 2, mg1, minf1, s)) || (rc = ctxop::miller_product(c, mg1, mg2, minf1, nullptr, 2, ml, s)) ||
        (rc = ctxop::gt_is_one(c, ml, 1, ml + 72, flag + 1, s)))
        return rc;
    return ctxop::fail(c, "k_kzg_finish", kzg_flag_finish(flag, all_ok, s));
}

}  // namespace zkp
