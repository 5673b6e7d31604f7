// cells_plan_check.cpp -- zkvm_pairings_amd/csrc/zkp_cells_plan.hpp (and the transforms of zkp_fk20_plan.hpp it drives) on the host, built with
// g++ -fsanitize=address,undefined (a stand-alone program: tests/test_cells_cpu.py compiles and runs it as a child process).
//   (no argument)  walks the plan at the ABI's maxima and one past them: argument limits, slices, group sizes, lanes, workspace bytes, every
//                  32-bit count; every scalar, base, partial and record a lane touches lies inside what the plan sizes; then RUNS the
//                  whole schedule of zkp_kzg_cells_setup and zkp_kzg_cells_batch - coefficient vectors, multiply-accumulate by groups,
//                  sum of the partials, both transforms, out - from the plan's functions alone over a toy group (the integers mod
//                  q = 15 2^27 + 1 under addition) against the quotient by X^l - c^l, for every group size the planner can return, both
//                  extensions and both orders; the verifier's table index and layout
//   shapes         reads "n log2_n log2_l" lines from stdin, prints "n log2_n log2_l g slice": the g the planner chooses and the polynomials of a slice
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../zkvm_pairings_amd/csrc/zkp_cells_plan.hpp"

namespace fk = zkp::fk20;
namespace cl = zkp::cells;

static long n_cases = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "cells plan_check: line %d: %s\n", __LINE__, #cond); \
            exit(1);                                                          \
        }                                                                     \
        n_cases++;                                                            \
    } while (0)

// ---- the toy field --------------------------------------------------------------------------------------------------------------------
static const uint64_t Q = 2013265921ull;   // 15 2^27 + 1, 31 generates the multiplicative group
static uint64_t qpow(uint64_t b, uint64_t e) {
    uint64_t r = 1;
    for (b %= Q; e; e >>= 1, b = b * b % Q)
        if (e & 1) r = r * b % Q;
    return r;
}
static uint64_t qinv(uint64_t a) { return qpow(a, Q - 2); }
static uint64_t root(unsigned k) { return qpow(31, (Q - 1) >> k); }
static std::vector<uint64_t> definition(const std::vector<uint64_t>& in, unsigned k, bool inverse, bool brv) {
    const size_t n = (size_t)1 << k;
    const uint64_t w = inverse ? qinv(root(k)) : root(k);
    std::vector<uint64_t> nat(n), out(n);
    for (size_t i = 0; i < n; i++) nat[i] = in[(inverse && brv) ? fk::bitrev((uint32_t)i, k) : i];   // the evaluation side is the bit-reversed one
    for (size_t i = 0; i < n; i++) {
        uint64_t acc = 0;
        for (size_t j = 0; j < n; j++) acc = (acc + nat[j] * qpow(w, i * j % n)) % Q;
        if (inverse) acc = acc * qinv(n % Q) % Q;
        out[(!inverse && brv) ? fk::bitrev((uint32_t)i, k) : i] = acc;
    }
    return out;
}

// ---- the schedule, from the plan's functions alone ---------------------------------------------------------------------------------------
struct Machine {
    std::vector<uint64_t> rec;
    std::vector<uint8_t> rec_inf;    // nothing here is ever "infinite" but a padded setup entry: kept to check SRC_INFINITY
    std::vector<uint64_t> table;     // w^i of the 2^table_log2-point domain
    unsigned table_log2 = 0;
    void tables(unsigned log2) {
        table_log2 = log2;
        table.assign((size_t)1 << log2, 1);
        for (size_t i = 1; i < table.size(); i++) table[i] = table[i - 1] * root(log2) % Q;
    }
    uint64_t& at(uint32_t r) {
        CHECK(r < rec.size());
        return rec[r];
    }
    void first(const fk::First& a, const std::vector<uint64_t>& wire, size_t wire_n) {
        CHECK(fk::count_ok(a.n_lane));
        for (uint32_t t = 0; t < a.n_lane; t++) {
            const uint32_t k = a.at.k, j = k ? t >> (k - 1) : t, e0 = k ? (t & fk::low_mask(k - 1)) << 1 : 0;
            const int64_t sa = fk::first_source(a, j, e0), sb = k ? fk::first_source(a, j, e0 + 1) : fk::SRC_INFINITY;
            if (a.mode == fk::SRC_REC) CHECK(sa != fk::SRC_INFINITY);      // k_g1ntt_first<SRC_REC> reads input A as a record without testing it
            auto get = [&](int64_t s) -> uint64_t {
                if (s == fk::SRC_INFINITY) return 0;
                if (a.mode == fk::SRC_REC) return at((uint32_t)s);
                CHECK((size_t)s < wire_n);
                return wire[(size_t)s];
            };
            const uint64_t A = get(sa), B = get(sb);
            const uint32_t r0 = fk::span_record(a.at, j, e0);
            if (!k) { at(r0) = A; continue; }
            at(r0 + 1) = (A + Q - B) % Q;
            at(r0) = (A + B) % Q;
        }
    }
    void stages(const fk::Span& sp, bool inverse) {
        for (uint32_t p = 1; p < sp.k; p++) {
            fk::Stage s;
            s.at = sp;
            s.p = p;
            s.inverse = inverse;
            s.tshift = table_log2 - sp.k;
            s.n_bfly = sp.n_vec << (sp.k - 1);
            CHECK(fk::count_ok(s.n_bfly) && fk::grid(s.n_bfly) * (uint64_t)fk::LANES >= s.n_bfly);
            std::vector<uint8_t> seen(rec.size(), 0);
            for (uint32_t t = 0; t < s.n_bfly; t++) {
                uint32_t r0, r1, tw;
                fk::stage_lane(s, t, &r0, &r1, &tw);
                CHECK(tw < table.size() && r0 < rec.size() && r1 < rec.size() && !seen[r0] && !seen[r1]);   // in place: nobody else's records
                seen[r0] = seen[r1] = 1;
                const uint64_t T = at(r1) * table[tw] % Q, A = at(r0);
                at(r1) = (A + Q - T) % Q;
                at(r0) = (A + T) % Q;
            }
        }
    }
    void out(const fk::Out& a, std::vector<uint64_t>& wire, uint64_t scale) {
        for (uint32_t t = 0; t < a.n_pt; t++) {
            uint32_t r;
            uint64_t slot;
            fk::out_lane(a, t, &r, &slot);
            CHECK(slot < wire.size());
            wire[slot] = a.scale ? at(r) * scale % Q : at(r);
        }
    }
};
static fk::First first_of(const fk::Span& at, uint32_t mode, bool perm, uint32_t src_off) {
    fk::First f;
    f.at = at;
    f.mode = mode;
    f.perm = perm;
    f.src_off = src_off;
    f.n_lane = at.k ? at.n_vec << (at.k - 1) : at.n_vec;
    return f;
}
static fk::Out out_of(const fk::Span& at, bool perm, bool scale) {
    fk::Out o;
    o.at = at;
    o.perm = perm;
    o.scale = scale;
    o.n_pt = at.n_vec << at.k;
    return o;
}
static uint64_t rnd(uint64_t& st) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    return (st >> 20) % Q;
}


// the whole producer over the toy group, with g = 2^s forced (the planner's own choice is checked in walk_limits)
static void run_cells(unsigned log2_n, unsigned log2_l, unsigned log2_ext, uint32_t n_poly, bool brv, uint32_t s, uint64_t tau) {
    const cl::Shape sh = cl::shape_of(log2_n, log2_l, log2_ext);
    const size_t n = (size_t)1 << log2_n, l = (size_t)1 << log2_l, k = (size_t)1 << sh.k, k2 = k << 1, big_m = (size_t)1 << sh.m, blk = (size_t)1 << sh.blk;
    uint64_t st = 7 + 31 * log2_n + 5 * log2_l + log2_ext + n_poly + s;
    std::vector<uint64_t> mono(n), f(n_poly * n);
    for (size_t i = 0; i < n; i++) mono[i] = qpow(tau, i);
    for (auto& v : f) v = rnd(st);
    if (n_poly > 1) for (size_t i = 0; i < n; i++) f[n + i] = i % 3 ? 0 : f[n + i];    // zero coefficients
    Machine m;
    m.tables(sh.k1 + 1);
    // the setup call: l vectors of 2 k, vector i the transform of (s_{N-l-1-i}, s_{N-2l-1-i}, .., identities)
    std::vector<uint64_t> setup(2 * n, ~0ull);
    {
        m.rec.assign(cl::setup_workspace_bytes(log2_n) / fk::REC_BYTES, 0);
        fk::Span sp;
        sp.k = sh.k1;
        sp.vs_log2 = sh.k1;
        sp.n_vec = (uint32_t)l;
        fk::First fi = first_of(sp, fk::SRC_CELLS, true, 0);
        fi.log2_l = log2_l;
        m.first(fi, mono, n);
        m.stages(sp, false);
        m.out(out_of(sp, false, false), setup, 0);
        for (size_t i = 0; i < l; i++) {
            std::vector<uint64_t> x(k2, 0);
            for (size_t e = 0; e + 2 <= k; e++) x[e] = mono[n - (e + 1) * l - 1 - i];
            const std::vector<uint64_t> want = definition(x, sh.k1, false, false);
            for (size_t t = 0; t < k2; t++) CHECK(setup[i * k2 + t] == want[t]);
        }
    }
    // a layout for exactly this call, but with the forced group size
    cl::Layout L = cl::layout(n_poly, log2_n, log2_l, log2_ext);
    CHECK(L.slice == n_poly && s <= log2_l && s <= cl::G_MAX_LOG2);
    const size_t parts = s == log2_l ? 0 : (n_poly * 2 * n) >> s;
    m.rec.assign(n_poly * blk, 0xdeadbeef);           // stale records: nothing may depend on them
    std::vector<uint64_t> part(parts, 0xdeadbeef), chat(n_poly * 2 * n);
    for (uint32_t id = 0; id < n_poly * 2 * n; id++) {          // k_cell_coeffs and the Fr transform
        const uint32_t t = id & fk::low_mask(sh.k1), i = (id >> sh.k1) & fk::low_mask(log2_l), j = id >> (sh.k1 + log2_l);
        const int64_t src = cl::coeff_source(t, i, sh.k, log2_l);
        CHECK(src < (int64_t)n);
        chat[id] = src < 0 ? 0 : f[j * n + src] * qinv(k2 % Q) % Q;
    }
    for (size_t v = 0; v < n_poly * l; v++) {
        const std::vector<uint64_t> one(chat.begin() + v * k2, chat.begin() + (v + 1) * k2), tr = definition(one, sh.k1, false, true);
        for (size_t t = 0; t < k2; t++) chat[v * k2 + t] = tr[t];
    }
    cl::Mac mac;
    mac.log2_l = log2_l;
    mac.k1 = sh.k1;
    mac.blk = sh.blk;
    mac.s = s;
    mac.n_lane = (uint32_t)((n_poly * 2 * n) >> s);
    CHECK(fk::count_ok(mac.n_lane));
    std::vector<uint8_t> used(chat.size(), 0);
    for (uint32_t id = 0; id < mac.n_lane; id++) {              // k_cell_mac
        uint32_t j, t, i0;
        cl::mac_lane(mac, id, &j, &t, &i0);
        CHECK(j < n_poly && t < k2 && i0 + (1u << s) <= l);
        uint64_t acc = 0;
        for (uint32_t q = 0; q < (1u << s); q++) {
            const uint64_t si = cl::mac_scalar(mac, j, t, i0 + q);
            const uint32_t bi = cl::mac_base(mac, t, i0 + q);
            CHECK(si < chat.size() && bi < setup.size() && !used[si]);
            used[si] = 1;
            acc = (acc + chat[si] * setup[bi]) % Q;
        }
        if (s == log2_l) m.at(cl::mac_record(mac, j, t)) = acc;
        else { CHECK(id < part.size()); part[id] = acc; }
    }
    for (uint8_t u : used) CHECK(u);
    if (s != log2_l) {                                          // k_cell_sum
        const uint32_t gl = log2_l - s, lanes = (uint32_t)(n_poly << sh.k1);
        for (uint32_t id = 0; id < lanes; id++) {
            uint64_t acc = 0;
            for (uint32_t q = 0; q < (1u << gl); q++) {
                CHECK(((size_t)id << gl) + q < part.size());
                acc = (acc + part[((size_t)id << gl) + q]) % Q;
            }
            m.at(((id >> sh.k1) << sh.blk) + (id & fk::low_mask(sh.k1))) = acc;
        }
    }
    fk::Span big, low;
    big.k = sh.k1;
    big.vs_log2 = sh.blk;
    big.n_vec = n_poly;
    m.first(first_of(big, fk::SRC_REC, false, 0), {}, 0);
    m.stages(big, true);
    for (uint32_t j = 0; j < n_poly; j++) CHECK(m.at((uint32_t)(j * blk + k - 1)) == 0);      // h_{k-1} is the identity
    low.k = sh.m;
    low.vs_log2 = sh.blk;
    low.off = 1u << sh.m;
    low.n_vec = n_poly;
    fk::First fi = first_of(low, fk::SRC_REC, true, 0);
    fi.src_len = (uint32_t)k;
    // the first stage reads records below k of a block and writes records from M on: no lane reads what another wrote
    for (uint32_t t = 0; t < fi.n_lane; t++) {
        const uint32_t j = sh.m ? t >> (sh.m - 1) : t, e0 = sh.m ? (t & fk::low_mask(sh.m - 1)) << 1 : 0;
        for (uint32_t e = e0; e < e0 + (sh.m ? 2u : 1u); e++) {
            const int64_t src = fk::first_source(fi, j, e);
            CHECK(src == fk::SRC_INFINITY || ((size_t)src >= j * blk && (size_t)src < j * blk + k));
            CHECK(fk::span_record(low, j, e) >= j * blk + big_m && fk::span_record(low, j, e) < (j + 1) * blk);
        }
    }
    m.first(fi, {}, 0);
    m.stages(low, false);
    std::vector<uint64_t> proof(n_poly * big_m, ~0ull);
    m.out(out_of(low, brv, false), proof, 0);
    const unsigned log2_d = log2_n + log2_ext;
    for (uint32_t j = 0; j < n_poly; j++)
        for (uint32_t slot = 0; slot < big_m; slot++) {
            const uint64_t c = qpow(root(log2_d), brv ? fk::bitrev(slot, sh.m) : slot), a = qpow(c, l);
            // q(tau) for q = (f - f mod (X^l - a)) / (X^l - a): synthetic division from the top
            std::vector<uint64_t> rem(f.begin() + j * n, f.begin() + (j + 1) * n);
            uint64_t qt = 0;
            for (size_t d = n; d-- > l;) {
                qt = (qt + rem[d] * qpow(tau, d - l)) % Q;
                rem[d - l] = (rem[d - l] + rem[d] * a) % Q;
            }
            CHECK(proof[j * big_m + slot] == qt);
        }
}

static void walk_limits() {
    CHECK(!cl::setup_args_bad(19, 19) && !cl::setup_args_bad(19, 0) && cl::setup_args_bad(20, 0) && cl::setup_args_bad(3, 4) && !cl::setup_args_bad(0, 0));
    CHECK(!cl::cells_args_bad(4, 19, 6, 1, 2) && cl::cells_args_bad(5, 19, 6, 1, 0) && cl::cells_args_bad(1, 20, 0, 0, 0) && cl::cells_args_bad(1, 3, 4, 0, 0));
    CHECK(cl::cells_args_bad(1, 3, 1, 2, 0) && cl::cells_args_bad(1, 3, 1, 0, 1) && cl::cells_args_bad(1, 3, 1, 0, 4) && cl::cells_args_bad(1, 3, 1, 0, -1));
    CHECK(!cl::cells_args_bad((size_t)1 << 21, 0, 0, 1, 0) && cl::cells_args_bad(((size_t)1 << 21) + 1, 0, 0, 0, 0) && !cl::cells_args_bad(0, 19, 19, 1, 2));
    for (unsigned log2_n = 0; log2_n <= cl::CELLS_MAX_LOG2; log2_n++)
        for (unsigned log2_l = 0; log2_l <= log2_n; log2_l++)
            for (unsigned ext = 0; ext < 2; ext++) {
                const size_t most = cl::CELLS_MAX_TOTAL >> log2_n;
                for (size_t n : {(size_t)1, most / 3 + 1, most}) {
                    if (n > most) continue;
                    const cl::Shape sh = cl::shape_of(log2_n, log2_l, ext);
                    const cl::Layout L = cl::layout(n, log2_n, log2_l, ext);
                    const size_t els = L.slice << (log2_n + 1), recs = L.slice << sh.blk;
                    CHECK(L.slice >= 1 && L.slice <= n && (els <= fk::SLICE_POINTS || L.slice == 1) && fk::count_ok(els) && fk::count_ok(recs));
                    CHECK(L.s <= cl::G_MAX_LOG2 && L.s <= log2_l && L.s == cl::group_log2(L.slice, log2_n, log2_l));
                    // the rule: g = 1 up to FULL_LANES lanes; beyond, the smallest g that brings them back, as far as l and G_MAX allow
                    CHECK(L.s == 0 ? (els <= cl::FULL_LANES || log2_l == 0) : (els >> (L.s - 1)) > cl::FULL_LANES);
                    CHECK((els >> L.s) <= cl::FULL_LANES || L.s == cl::G_MAX_LOG2 || L.s == log2_l);
                    const size_t parts = L.s == log2_l ? 0 : els >> L.s;
                    CHECK(L.rec == 0 && L.part % 256 == 0 && L.fr % 256 == 0 && L.part >= recs * fk::REC_BYTES && L.fr >= L.part + parts * fk::REC_BYTES &&
                          L.total >= L.fr + els * 32);
                    CHECK(L.total <= (L.slice == 1 ? ((size_t)2 << log2_n) * (32 + 192 + 384) + 768 : ((size_t)152 << 20) + 768));
                    CHECK(!fk::g1ntt_args_bad(L.slice, sh.k1, 0) && !fk::g1ntt_args_bad(L.slice, sh.m, 0) && sh.m <= sh.k1);
                    cl::Mac mac;
                    mac.log2_l = log2_l;
                    mac.k1 = sh.k1;
                    mac.blk = sh.blk;
                    mac.s = L.s;
                    mac.n_lane = (uint32_t)(els >> L.s);
                    uint32_t j, t, i0;
                    cl::mac_lane(mac, mac.n_lane - 1, &j, &t, &i0);
                    const uint32_t last = i0 + (1u << L.s) - 1;
                    CHECK(j == L.slice - 1 && t == (2u << sh.k) - 1 && last == (1u << log2_l) - 1);
                    CHECK(cl::mac_scalar(mac, j, t, last) == els - 1 && cl::mac_base(mac, t, last) < ((size_t)2 << log2_n) && cl::mac_record(mac, j, t) < recs);
                    cl::mac_lane(mac, 0, &j, &t, &i0);
                    CHECK(j == 0 && t == 0 && i0 == 0);
                }
            }
    // First::src_len's precondition for every shape the producer builds: perm, src_len = k >= M / 2, so input A is always a record
    for (unsigned m = 0; m <= cl::CELLS_MAX_LOG2 + 1; m++)
        for (unsigned ext = 0; ext < 2 && ext <= m; ext++) {
            fk::Span low;
            low.k = m;
            low.vs_log2 = m + 1;
            low.off = 1u << m;
            low.n_vec = 1;
            fk::First fi = first_of(low, fk::SRC_REC, true, 0);
            fi.src_len = 1u << (m - ext);
            CHECK(!m || fi.src_len >= (1u << (m - 1)));
            for (uint32_t e0 : {0u, 2u, (1u << m) - 2u})
                if (m && e0 < (1u << m)) CHECK(fk::first_source(fi, 0, e0) != fk::SRC_INFINITY && fk::first_source(fi, 0, e0) < (int64_t)fi.src_len);
        }
    // the stride vectors on their own: every coefficient but f_0 .. f_{l-1}'s mirror positions is used exactly once over the l strides
    for (unsigned log2_n = 0; log2_n <= 6; log2_n++)
        for (unsigned log2_l = 0; log2_l <= log2_n; log2_l++) {
            const uint32_t n = 1u << log2_n, l = 1u << log2_l, k = n / l;
            std::vector<int> hits(n, 0);
            for (uint32_t i = 0; i < l; i++)
                for (uint32_t t = 0; t < 2 * k; t++) {
                    const int64_t s = cl::coeff_source(t, i, log2_n - log2_l, log2_l);
                    if (s < 0) continue;
                    CHECK(s < (int64_t)n && (t == 0) == (s == (int64_t)n - 1 - i));
                    hits[s]++;
                }
            for (uint32_t c = 0; c < n; c++) CHECK(hits[c] == (k == 1 ? (c >= n - l) : (c >= l)));     // k = 1: (f_{N-1-i}, 0); else f_0 .. f_{l-1} never
            uint32_t finite = 0;
            for (uint32_t i = 0; i < l; i++)
                for (uint32_t e = 0; e < 2 * k; e++) {
                    const int64_t s = fk::cells_setup_source(log2_l, log2_n - log2_l + 1, i, e);
                    if (s == fk::SRC_INFINITY) continue;
                    finite++;
                    CHECK(e + 2 <= k && s == (int64_t)(n - (e + 1) * l - 1 - i));
                }
            CHECK(finite == l * (k - 1));
        }
    // the verifier: limits, the table index of c^-i, a layout at the maxima
    CHECK(!cl::verify_args_bad(0, 20, 15, 14) && cl::verify_args_bad(1, 21, 3, 0) && cl::verify_args_bad(1, 3, 4, 0) && cl::verify_args_bad(1, 20, 16, 0));
    CHECK(cl::verify_args_bad(1, 3, 1, 1) && cl::verify_args_bad(1, 3, 1, 16) && !cl::verify_args_bad((size_t)1 << 21, 20, 5, 2) &&
          cl::verify_args_bad(((size_t)1 << 21) + 1, 20, 0, 0) && cl::verify_args_bad(((size_t)1 << 11) + 1, 20, 15, 0) && !cl::verify_args_bad((size_t)1 << 11, 20, 15, 0));
    for (unsigned log2_d = 0; log2_d <= 7; log2_d++)
        for (uint32_t mm = 0; mm < (1u << log2_d); mm++)
            for (uint32_t i = 0; i < (1u << log2_d); i++) {
                const uint32_t e = cl::inverse_power_index(mm, i, log2_d);
                CHECK(e < (1u << log2_d) && qpow(root(log2_d), e) * qpow(root(log2_d), (uint64_t)mm * i) % Q == 1);
            }
    CHECK(cl::inverse_power_index((1u << 20) - 1, (1u << 15) - 1, 20) < (1u << 20));
    for (int flags : {0, 4, 8, 12}) {
        const cl::VerifyLayout V = cl::verify_layout((size_t)1 << 21, 5, flags, 0, 4096);
        CHECK(V.n_status == ((flags & 4) ? 0 : (size_t)1 << 22) + ((flags & 8) ? 0 : 34) && V.total % 256 == 0 && V.coef >= V.st + V.n_status);
        CHECK(V.ms >= V.coef + ((size_t)1 << 26) * 32 && V.mp >= V.ms + 2 * (((size_t)1 << 22) + 32) * 32 && V.total >= V.ml + 2 * 576);
        CHECK(2 * (2 * ((size_t)1 << 21) + 32) <= ((size_t)1 << 24));      // the two-row MSM stays inside the MSM's limit
    }
}

static int shapes_mode() {
    unsigned long n;
    unsigned log2_n, log2_l;
    while (scanf("%lu %u %u", &n, &log2_n, &log2_l) == 3) {
        if (cl::cells_args_bad(n, log2_n, log2_l, 0, 0) || !n) return 1;
        const cl::Layout L = cl::layout(n, log2_n, log2_l, 1);
        printf("%lu %u %u %u %zu\n", n, log2_n, log2_l, 1u << L.s, L.slice);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "shapes")) return shapes_mode();
    walk_limits();
    for (unsigned log2_n = 0; log2_n <= 6; log2_n++)
        for (unsigned log2_l = 0; log2_l <= log2_n; log2_l++)
            for (unsigned ext = 0; ext < 2; ext++)
                for (uint32_t s = 0; s <= cl::G_MAX_LOG2 && s <= log2_l; s++)
                    for (uint32_t n_poly : {1u, 3u}) {
                        if (log2_n > 4 && n_poly > 1 && s) continue;
                        run_cells(log2_n, log2_l, ext, n_poly, (log2_n + log2_l + s + n_poly) & 1, s, 123456789);
                        if (log2_n == 3) run_cells(log2_n, log2_l, ext, n_poly, !((log2_n + log2_l + s + n_poly) & 1), s, 987654321);
                    }
    printf("cells plan_check ok: %ld cases\n", n_cases);
    return 0;
}
