// zkp_poly_plan.hpp -- the PURE index arithmetic of the batched Fr NTT (zkp_fr_ntt_batch) and of the KZG opening (zkp_kzg_open_batch):
// the argument limits, the pass plan of a log2_n, the element a (pass, workgroup, tile slot) stands for, the LDS slot it is kept in,
// the rounds of a pass, the twiddle index of a butterfly, the store permutation, grids and workspace bytes.  No HIP type, no
// allocation, no I/O.  zkp_poly.hip compiles this text for the device; tests/poly_plan_check.cpp compiles it with
// g++ -fsanitize=address,undefined and RUNS every pass of the transform on the host from these functions alone.
//
// The transform.  An index of a polynomial has k = log2_n bits.  A radix-2 stage "on bit p" pairs the elements whose indices differ in
// bit p; its twiddle is w^((i mod 2^p) << (k - 1 - p)).  Decimation in frequency (DIF) runs the stages from bit k - 1 down to bit 0, takes
// natural order and leaves element i holding X[bitrev(i)]; decimation in time (DIT) runs them upwards, takes bit-reversed order and
// leaves natural order.  Both work in place, which is what a PASS exploits: a pass owns a range [lo, lo + kp) of bits, a workgroup
// takes a TILE of 2^t elements that holds every combination of those bits, runs the kp stages in LDS and writes the elements back
// where it found them.  The t - kp other bits of a tile ("companions") are chosen so that global runs are long:
//   row pass     lo = 0: the tile is 2^t consecutive elements (several polynomials when k < t)
//   column pass  lo > 0: cl = t - kp LOW bits, so each of the 2^kp strided rows of the tile is a run of 2^cl >= 4 elements (128 B)
//   top pass     lo = 0, kp = t - 2, the companions are the TOP two bits of the index.  It is the last pass of a transform that must
//                leave natural order (no ZKP_NTT_BITREV): element i goes to bitrev(i), and the four elements of a tile that share
//                their low bits land side by side - a 128-byte run.  Its read set and write set differ, so it reads the workspace
//   with ZKP_NTT_BITREV   forward = DIF, inverse = DIT, all passes in place, no workspace: k <= t one pass, k <= 2 t - 2 two, else three
//   without               DIF both ways; k <= t one pass (the permutation happens between LDS and the store), k <= 2 t - 4 two, else three
// For t = 10: BITREV one pass to 2^10, two to 2^18, three beyond; natural order one to 2^10, two to 2^16, three beyond.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZKP_POLY_HD __host__ __device__ __forceinline__
#else
#define ZKP_POLY_HD inline
#endif

namespace zkp {
namespace poly {

constexpr unsigned TILE_LOG2 = 10;               // t of the product: 1024 elements = 32 KiB of LDS, four per thread
constexpr unsigned TPB = 256;
constexpr unsigned NTT_MAX_LOG2 = 20;
constexpr size_t NTT_MAX_TOTAL = (size_t)1 << 26;    // n_poly * N
constexpr int NTT_INVERSE = 1, NTT_BITREV = 2, NTT_COSET = 4, NTT_ALL_FLAGS = 7;
constexpr unsigned COSET_LOG2 = 10;              // 7^e = lo[e mod 2^10] hi[e >> 10]: two tables of 2^10, and the same for 7^-1
constexpr size_t COSET_BYTES = (size_t)4 * 32 << COSET_LOG2;
constexpr int MAX_PASSES = 16;                   // of a plan with a small t (the host replay); the product needs three
constexpr size_t OPEN_MAX_TERMS = (size_t)1 << 24;   // n * N of the opening: the MSM's term limit
constexpr size_t OPEN_SLICE_TERMS = (size_t)1 << 22; // evaluations of one slice of the opening
constexpr int OPEN_ALL_FLAGS = 1;                // ZKP_FR_EVAL_BITREV

constexpr bool ntt_args_bad(size_t n_poly, unsigned log2_n, int flags) {
    return log2_n > NTT_MAX_LOG2 || (flags & ~NTT_ALL_FLAGS) || n_poly > (NTT_MAX_TOTAL >> log2_n);
}
constexpr bool open_args_bad(size_t n, unsigned log2_n, int flags) {
    return log2_n > NTT_MAX_LOG2 || (flags & ~OPEN_ALL_FLAGS) || n > (OPEN_MAX_TERMS >> log2_n);
}
// the opening runs in slices of whole polynomials: at most OPEN_SLICE_TERMS evaluations each, and at least one polynomial
constexpr size_t open_slice(size_t n, unsigned log2_n) {
    const size_t per = (OPEN_SLICE_TERMS >> log2_n) ? (OPEN_SLICE_TERMS >> log2_n) : 1;
    return n < per ? n : per;
}

// the low `bits` bits of v reversed (bits <= 32; 0 for bits == 0)
ZKP_POLY_HD uint32_t bitrev(uint32_t v, unsigned bits) {
    if (!bits) return 0;
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - bits);
}
ZKP_POLY_HD uint32_t low_mask(unsigned bits) { return bits >= 32 ? 0xffffffffu : (1u << bits) - 1u; }

enum { KIND_PLACE = 0, KIND_TOP = 1 };           // a pass that writes where it read / the top pass
enum { STORE_SAME = 0, STORE_BITREV = 1, STORE_TOP = 2 };

// what a launch receives by value
struct Pass {
    uint32_t k = 0, t = 0;        // log2 of the polynomial and of the tile
    uint32_t lo = 0, kp = 0;      // the pass's stages: bits lo .. lo + kp - 1
    uint32_t cl = 0, ch = 0;      // tile bits below / above the kp transform bits (cl + kp + ch = t)
    uint32_t kind = KIND_PLACE, store = STORE_SAME;
    uint32_t dit = 0, inverse = 0;
    uint32_t coset_in = 0;        // multiply element i by 7^i while loading (forward coset, first pass)
    uint32_t coset_out = 0;       // multiply element i by 7^-i while storing (inverse coset, last pass)
    uint32_t scale = 0;           // multiply by 2^-k while storing (inverse, last pass)
    uint32_t total = 0;           // n_poly << k
};
struct Plan {
    int n_pass = 0;
    bool ok = false;
    bool workspace = false;       // every pass but the last writes the workspace (the top pass cannot run in place)
    Pass pass[MAX_PASSES];
};

inline size_t ntt_tiles(size_t n_poly, unsigned log2_n, unsigned t = TILE_LOG2) { return ((n_poly << log2_n) + ((size_t)1 << t) - 1) >> t; }
// device bytes the transform needs beside its operands: a copy of the data when the plan ends in a top pass
inline size_t ntt_workspace_bytes(size_t n_poly, unsigned log2_n, int flags, unsigned t = TILE_LOG2) {
    return (!(flags & NTT_BITREV) && log2_n > t) ? (n_poly << log2_n) * 32 : 0;
}

// n_poly >= 1 and !ntt_args_bad; t >= 4
inline Plan make_plan(size_t n_poly, unsigned k, int flags, unsigned t = TILE_LOG2) {
    Plan P;
    const bool inverse = flags & NTT_INVERSE, brv = flags & NTT_BITREV, coset = flags & NTT_COSET;
    const bool dit = brv && inverse;
    Pass base;
    base.k = k;
    base.t = t;
    base.dit = dit;
    base.inverse = inverse;
    base.total = (uint32_t)(n_poly << k);
    // the passes by ascending bit range
    Pass asc[MAX_PASSES];
    int n = 0;
    const bool top = !brv && k > t;
    const unsigned first = k <= t ? k : (top ? t - 2 : t);    // the bits of the pass at lo = 0
    asc[n] = base;
    asc[n].lo = 0;
    asc[n].kp = first;
    asc[n].cl = 0;
    asc[n].ch = t - first;
    asc[n].kind = top ? KIND_TOP : KIND_PLACE;
    n++;
    const unsigned rem = k - first, cap = t - 2;
    const unsigned np = (rem + cap - 1) / cap;
    if ((int)np + 1 > MAX_PASSES) return P;
    unsigned lo = first;
    for (unsigned j = 0; j < np; j++) {
        const unsigned kp = rem / np + (j < rem % np ? 1 : 0);   // the larger ones first: the lowest column pass needs lo >= cl
        asc[n] = base;
        asc[n].lo = lo;
        asc[n].kp = kp;
        asc[n].cl = t - kp < lo ? t - kp : lo;
        asc[n].ch = t - kp - asc[n].cl;
        if (asc[n].cl < 2) return P;
        lo += kp;
        n++;
    }
    P.n_pass = n;
    for (int i = 0; i < n; i++) P.pass[i] = dit ? asc[i] : asc[n - 1 - i];   // DIF starts at the top bit
    Pass& last = P.pass[n - 1];
    if (!brv) last.store = top ? STORE_TOP : STORE_BITREV;
    if (inverse) last.scale = 1;
    if (coset && inverse) last.coset_out = 1;
    if (coset && !inverse) P.pass[0].coset_in = 1;
    P.workspace = top;
    P.ok = true;
    return P;
}

// ---- a tile -----------------------------------------------------------------------------------------------------------------------
// tile element e (t bits: cl low companions | kp transform bits | ch high companions) of workgroup wg -> the flat index into the
// n_poly x N array.  The polynomial's own index is the low k bits.
ZKP_POLY_HD uint64_t element_index(const Pass& a, uint32_t wg, uint32_t e) {
    const uint32_t tr = (e >> a.cl) & low_mask(a.kp);
    const uint64_t eh = e >> (a.cl + a.kp);
    if (a.kind == KIND_TOP) {   // cl = 0, the ch companions are bits k - ch .. k - 1
        const uint32_t mb = a.k - a.kp - a.ch;
        const uint64_t mid = wg & low_mask(mb), poly = wg >> mb;
        return tr | (mid << a.kp) | (eh << (a.k - a.ch)) | (poly << a.k);
    }
    const uint32_t el = e & low_mask(a.cl), wb = a.lo - a.cl;
    const uint64_t wl = wg & low_mask(wb), wh = wg >> wb;
    return el | (wl << a.cl) | ((uint64_t)tr << a.lo) | (((wh << a.ch) | eh) << (a.lo + a.kp));
}
// store slot u of the tile (thread q stores slots q, q + threads, ...: consecutive slots are consecutive addresses) -> the tile
// element that is written there and the flat index it is written to
ZKP_POLY_HD void store_map(const Pass& a, uint32_t wg, uint32_t u, uint32_t* e, uint64_t* index) {
    if (a.store == STORE_SAME) {
        *e = u;
        *index = element_index(a, wg, u);
    } else if (a.store == STORE_BITREV) {   // one row pass holds whole polynomials: slot u takes the element of bit-reversed index
        *e = (u & ~low_mask(a.k)) | bitrev(u & low_mask(a.k), a.k);
        *index = element_index(a, wg, u);
    } else {                                // y: the reversed top companions, x: the reversed transform bits
        const uint32_t y = u & low_mask(a.ch), x = u >> a.ch, mb = a.k - a.kp - a.ch;
        const uint64_t mid = wg & low_mask(mb), poly = wg >> mb;
        *e = (bitrev(y, a.ch) << a.kp) | bitrev(x, a.kp);
        *index = y | ((uint64_t)bitrev((uint32_t)mid, mb) << a.ch) | ((uint64_t)x << (a.k - a.kp)) | (poly << a.k);
    }
}
// where tile element e lives in LDS (word w of it at w * 2^t + slot).  In every round and in the load and store phases the 32 lanes
// of a group then touch 32 different banks: bits 5 and 6 of e - which a round's lanes vary in place of the two bits they hold in
// registers - are folded into the low five bits.
ZKP_POLY_HD uint32_t lds_slot(uint32_t e) { return e ^ (((e >> 6) & 1u) * 21u) ^ (((e >> 5) & 1u) * 10u); }

// ---- the rounds of a pass: up to two stages on the four elements a thread holds ---------------------------------------------------
struct Round {
    uint32_t pos = 0;      // the thread's four elements differ in tile bits pos and pos + 1
    uint32_t lo = 0, hi = 0;   // run the stage on bit pos / on bit pos + 1
};
ZKP_POLY_HD uint32_t n_rounds(const Pass& a) { return (a.kp + 1) / 2; }
ZKP_POLY_HD Round round_of(const Pass& a, uint32_t r) {
    Round R;
    const uint32_t b0 = a.cl, b1 = a.cl + a.kp;   // the transform bits of the tile: b0 .. b1 - 1
    uint32_t single = 0;
    bool one = false;
    if (a.dit) {
        R.pos = b0 + 2 * r;
        one = R.pos + 1 >= b1;
        single = R.pos;
    } else {
        one = b0 + 2 * (r + 1) > b1;
        R.pos = one ? b0 : b1 - 2 * (r + 1);
        single = b0;
    }
    if (!one) {
        R.lo = R.hi = 1;
    } else if (single + 1 < a.t) {
        R.pos = single;
        R.lo = 1;
    } else {
        R.pos = single - 1;
        R.hi = 1;
    }
    return R;
}
// element j (0 .. 3) of thread q in a round: j's two bits go in at pos
ZKP_POLY_HD uint32_t round_element(const Round& R, uint32_t q, uint32_t j) {
    return ((q >> R.pos) << (R.pos + 2)) | (j << R.pos) | (q & low_mask(R.pos));
}
// the twiddle of the butterfly on tile bit b whose upper element (bit clear) is tile element e: an index into the table w^i of the
// 2^k-point domain; 0 means "one"
ZKP_POLY_HD uint32_t twiddle_index(const Pass& a, uint32_t wg, uint32_t e, uint32_t b) {
    const uint32_t p = a.lo + b - a.cl;
    const uint32_t i = (uint32_t)element_index(a, wg, e) & low_mask(a.k);
    const uint32_t ex = (i & low_mask(p)) << (a.k - 1 - p);
    return a.inverse ? ((1u << a.k) - ex) & low_mask(a.k) : ex;
}

}  // namespace poly
}  // namespace zkp
