// fk20_plan_check.cpp -- zkvm_pairings_amd/csrc/zkp_fk20_plan.hpp on the host, built with g++ -fsanitize=address,undefined (a stand-alone
// program: tests/test_fk20_cpu.py compiles and runs it as a child process).
//   (no argument)  walks the plan at the ABI's maxima and one past them: argument limits, slices, grids, workspace bytes, every 32-bit
//                  count; every record a lane touches lies inside the workspace the plan sizes, every wire index inside the call's arrays;
//                  then RUNS the schedule - first stage, twiddled stages, out - from the plan's functions alone over a toy group (the
//                  integers mod q = 15 2^27 + 1 under addition, twiddles from that field) against the transform's definition, for every
//                  flag combination, and the whole FK20 pipeline against the quotient formula
//   split          reads 64-digit hex scalars from stdin, prints "a b" (hex) of split_z2 for each: the table-building kernel's arithmetic
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../zkvm_pairings_amd/csrc/zkp_fk20_plan.hpp"

namespace fk = zkp::fk20;

static long n_cases = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "fk20 plan_check: line %d: %s\n", __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
        n_cases++;                                                           \
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

static void run_ntt(unsigned k, uint32_t n_vec, int flags, unsigned table_log2) {
    const bool inverse = flags & fk::NTT_INVERSE, brv = flags & fk::NTT_BITREV;
    const size_t n = (size_t)1 << k;
    uint64_t st = 17 * k + n_vec + flags;
    std::vector<uint64_t> in(n_vec * n), got(n_vec * n, ~0ull);
    for (auto& v : in) v = rnd(st);
    Machine m;
    m.tables(table_log2);
    CHECK(fk::slice_vectors(n_vec, k) == n_vec);
    m.rec.assign(fk::g1ntt_workspace_bytes(n_vec, k) / fk::REC_BYTES, 0);
    fk::Span sp;
    sp.k = k;
    sp.vs_log2 = k;
    sp.n_vec = n_vec;
    m.first(first_of(sp, fk::SRC_WIRE, !(inverse && brv), 0), in, in.size());
    m.stages(sp, inverse);
    m.out(out_of(sp, !inverse && brv, inverse && k), got, qinv(n % Q));
    for (uint32_t j = 0; j < n_vec; j++) {
        const std::vector<uint64_t> one(in.begin() + j * n, in.begin() + (j + 1) * n), want = definition(one, k, inverse, brv);
        for (size_t i = 0; i < n; i++) CHECK(got[j * n + i] == want[i]);
    }
}

static void run_fk20(unsigned k, uint32_t n_poly, bool brv, uint64_t tau) {
    const unsigned k1 = k + 1;
    const size_t n = (size_t)1 << k, n2 = n << 1;
    uint64_t st = 99 + k + n_poly;
    std::vector<uint64_t> mono(n), f(n_poly * n);
    for (size_t i = 0; i < n; i++) mono[i] = qpow(tau, i);
    for (auto& v : f) v = rnd(st);
    Machine m;
    m.tables(k1 + 1);    // a table larger than the transform: the stride
    // the setup call
    std::vector<uint64_t> setup(n2, ~0ull);
    {
        m.rec.assign(fk::g1ntt_workspace_bytes(1, k1) / fk::REC_BYTES, 0);
        fk::Span sp;
        sp.k = k1;
        sp.vs_log2 = k1;
        sp.n_vec = 1;
        m.first(first_of(sp, fk::SRC_SETUP, true, 0), mono, n);
        m.stages(sp, false);
        m.out(out_of(sp, false, false), setup, 0);
        std::vector<uint64_t> x(n2, 0);
        for (size_t e = 0; e + 2 <= n; e++) x[e] = mono[n - 2 - e];
        CHECK(setup == definition(x, k1, false, false));
    }
    const fk::Fk20Layout L = fk::fk20_layout(n_poly, k);
    CHECK(L.slice == n_poly && L.fr >= (n_poly << k1) * fk::REC_BYTES && L.total >= L.fr + (n_poly << k1) * 32);
    m.rec.assign(L.fr / fk::REC_BYTES, 0);
    for (uint32_t j = 0; j < n_poly; j++) {
        std::vector<uint64_t> c(n2, 0);
        for (uint32_t i = 0; i < n2; i++) {
            const int64_t s = fk::coeff_source(i, k);
            CHECK(s < (int64_t)n);
            if (s >= 0) c[i] = f[j * n + s] * qinv(n2 % Q) % Q;
        }
        const std::vector<uint64_t> chat = definition(c, k1, false, true);     // the Fr transform, bit-reversed evaluations
        for (uint32_t t = 0; t < n2; t++) m.at((uint32_t)(j * n2 + t)) = chat[t] * setup[fk::bitrev(t, k1)] % Q;   // k_fk20_mul
    }
    fk::Span big, low;
    big.k = k1;
    big.vs_log2 = k1;
    big.n_vec = n_poly;
    m.first(first_of(big, fk::SRC_REC, false, 0), {}, 0);
    m.stages(big, true);
    for (uint32_t j = 0; j < n_poly; j++) CHECK(m.at((uint32_t)(j * n2 + n - 1)) == 0);     // h_{N-1} is the identity
    low.k = k;
    low.vs_log2 = k1;
    low.off = 1u << k;
    low.n_vec = n_poly;
    m.first(first_of(low, fk::SRC_REC, true, 0), {}, 0);
    m.stages(low, false);
    std::vector<uint64_t> proof(n_poly * n, ~0ull);
    m.out(out_of(low, brv, false), proof, 0);
    for (uint32_t j = 0; j < n_poly; j++) {
        uint64_t ft = 0;
        for (size_t i = n; i-- > 0;) ft = (ft * tau + f[j * n + i]) % Q;
        for (uint32_t slot = 0; slot < n; slot++) {
            const uint64_t x = qpow(root(k), brv ? fk::bitrev(slot, k) : slot);
            uint64_t y = 0;
            for (size_t i = n; i-- > 0;) y = (y * x + f[j * n + i]) % Q;
            CHECK(proof[j * n + slot] == (ft + Q - y) % Q * qinv((tau + Q - x) % Q) % Q);
        }
    }
}

static void walk_limits() {
    CHECK(!fk::g1ntt_args_bad(0, 0, 0) && !fk::g1ntt_args_bad(4, 20, 3) && fk::g1ntt_args_bad(5, 20, 0) && fk::g1ntt_args_bad(1, 21, 0));
    CHECK(!fk::g1ntt_args_bad((size_t)1 << 22, 0, 0) && fk::g1ntt_args_bad(((size_t)1 << 22) + 1, 0, 0));
    CHECK(fk::g1ntt_args_bad(1, 3, 4) && fk::g1ntt_args_bad(1, 3, 8) && fk::g1ntt_args_bad(1, 3, -1) && fk::g1ntt_args_bad(~(size_t)0, 1, 0));
    CHECK(!fk::setup_args_bad(19) && fk::setup_args_bad(20) && !fk::setup_args_bad(0));
    CHECK(!fk::fk20_args_bad(4, 19, 2) && fk::fk20_args_bad(5, 19, 0) && fk::fk20_args_bad(1, 20, 0) && fk::fk20_args_bad(1, 3, 1) &&
          fk::fk20_args_bad(1, 3, 4) && !fk::fk20_args_bad((size_t)1 << 21, 0, 0) && fk::fk20_args_bad(((size_t)1 << 21) + 1, 0, 0));
    // every legal (n_vec, log2_n) at the edges: slices of whole vectors, a bounded workspace, 32-bit counts
    for (unsigned k = 0; k <= fk::G1NTT_MAX_LOG2; k++) {
        const size_t most = fk::G1NTT_MAX_TOTAL >> k;
        for (size_t n_vec : {(size_t)1, most / 2 + 1, most}) {
            if (!n_vec || n_vec > most) continue;
            const size_t sl = fk::slice_vectors(n_vec, k), pts = sl << k;
            CHECK(sl >= 1 && sl <= n_vec && (pts <= fk::SLICE_POINTS || sl == 1));
            CHECK(fk::g1ntt_workspace_bytes(n_vec, k) == pts * fk::REC_BYTES && fk::g1ntt_workspace_bytes(n_vec, k) <= ((size_t)192 << 20));
            CHECK(fk::count_ok(pts) && (uint64_t)fk::grid(pts) * fk::LANES >= pts && (uint64_t)fk::grid(pts) * fk::LANES < pts + fk::LANES);
            // the last lane of the last stage and of the out kernel stay inside the slice
            fk::Span sp;
            sp.k = k;
            sp.vs_log2 = k;
            sp.n_vec = (uint32_t)sl;
            if (k >= 2) {
                fk::Stage s;
                s.at = sp;
                s.p = k - 1;
                s.inverse = 1;
                s.tshift = 0;
                s.n_bfly = (uint32_t)(pts >> 1);
                uint32_t r0, r1, tw;
                fk::stage_lane(s, s.n_bfly - 1, &r0, &r1, &tw);
                CHECK(r0 < r1 && r1 == pts - 1 && tw < ((size_t)1 << k));
            }
            uint32_t r;
            uint64_t slot;
            const fk::Out o = out_of(sp, true, false);
            fk::out_lane(o, o.n_pt - 1, &r, &slot);
            CHECK(r == pts - 1 && slot < pts);
            const fk::First fi = first_of(sp, fk::SRC_WIRE, true, 0);
            CHECK(fi.n_lane >= 1 && fk::first_source(fi, (uint32_t)sl - 1, (uint32_t)((size_t)1 << k) - 1) < (int64_t)pts);
        }
    }
    for (unsigned k = 0; k <= fk::FK20_MAX_LOG2; k++) {
        const size_t most = fk::FK20_MAX_TOTAL >> k;
        for (size_t n : {(size_t)1, most}) {
            const fk::Fk20Layout L = fk::fk20_layout(n, k);
            const size_t pts = L.slice << (k + 1);
            CHECK(L.slice >= 1 && L.slice <= n && (pts <= fk::SLICE_POINTS || L.slice == 1) && fk::count_ok(pts));
            CHECK(L.rec == 0 && L.fr % 256 == 0 && L.fr >= pts * fk::REC_BYTES && L.total >= L.fr + pts * 32 && L.total <= ((size_t)225 << 20));
            CHECK(!zkp::fk20::g1ntt_args_bad(1, k + 1, 0));     // the transforms of size 2 N are legal ones
        }
        CHECK(fk::split_table_bytes(k + 1) == ((size_t)32 << (k + 1)));
    }
    // the setup vector and the coefficient vector on their own
    for (unsigned k = 0; k <= 6; k++) {
        const uint32_t n = 1u << k;
        fk::Span sp;
        sp.k = k + 1;
        sp.vs_log2 = k + 1;
        sp.n_vec = 1;
        const fk::First fi = first_of(sp, fk::SRC_SETUP, false, 0);
        uint32_t finite = 0;
        for (uint32_t e = 0; e < 2 * n; e++) {
            const int64_t s = fk::first_source(fi, 0, e);
            if (s == fk::SRC_INFINITY) continue;
            finite++;
            CHECK(e + 2 <= n && s == (int64_t)(n - 2 - e));
        }
        CHECK(finite == (n >= 2 ? n - 1 : 0));
        uint32_t used = 0;
        for (uint32_t i = 0; i < 2 * n; i++) {
            const int64_t s = fk::coeff_source(i, k);
            if (s < 0) continue;
            used++;
            CHECK(i == 0 ? s == (int64_t)n - 1 : (s >= 1 && s + 2 <= (int64_t)n && i == n + 1 + (uint32_t)s));
        }
        CHECK(used == (n >= 2 ? n - 1 : 1));
    }
}

static int split_mode() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        if (strlen(line) < 64) continue;
        uint32_t s[8], a[4], b[4];
        for (int w = 0; w < 8; w++) {
            char part[9];
            memcpy(part, line + 8 * (7 - w), 8);
            part[8] = 0;
            s[w] = (uint32_t)strtoul(part, nullptr, 16);
        }
        fk::split_z2(s, a, b);
        printf("%08x%08x%08x%08x %08x%08x%08x%08x\n", a[3], a[2], a[1], a[0], b[3], b[2], b[1], b[0]);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "split")) return split_mode();
    walk_limits();
    for (unsigned k = 0; k <= 8; k++)
        for (uint32_t n_vec : {1u, 3u})
            for (int flags = 0; flags < 4; flags++) {
                if (k > 6 && n_vec > 1) continue;
                run_ntt(k, n_vec, flags, k);
                if (k == 3) run_ntt(k, n_vec, flags, k + 2);
            }
    for (unsigned k = 0; k <= 6; k++)
        for (uint32_t n_poly : {1u, 3u})
            for (int brv = 0; brv < 2; brv++) run_fk20(k, n_poly, brv, 123456789);
    printf("fk20 plan_check ok: %ld cases\n", n_cases);
    return 0;
}
