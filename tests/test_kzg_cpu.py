"""CPU gate for the batched Fr inversion, the barycentric evaluation and the batch KZG opening verifier: the additions to csrc/zkp_fr.hpp
(pow, the roots of unity, 2^-k, the inversion's per-thread pieces) built for the host with g++ and UBSan and compared with Python integers;
the run / scan / back-sweep schedule of zkp_kzg.hip replayed on the host from those pieces, with its Montgomery products counted; the
planner (csrc/zkp_kzg_plan.hpp) under ASan and UBSan; struct layouts and flags in the header, ctypes and Rust; the new kernels' registers;
the folded equation and the barycentric formula as Python models."""
import ctypes
import json
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MONT = 1 << 256
Z2 = 0xD201000000010000 ** 2          # z^2 of the curve parameter: r_i = a_i + b_i z^2
VK_FIELDS = ["g1", "g2", "tau_g2"]
BATCH_FIELDS = ["n", "c", "inf_c", "proof", "inf_proof", "z", "y"]
NEW = ["zkp_fr_invert_batch", "zkp_fr_invert_batch_dev", "zkp_fr_eval_batch", "zkp_fr_eval_batch_dev", "zkp_kzg_verify_batch", "zkp_kzg_verify_batch_dev"]

# The host replay of zkp_kzg.hip's inversion: the same per-thread pieces (inv_run_prefix / inv_run_back), the same tree, the same two
# Hillis-Steele scans restricted to the threads that hold data, the same middle level - threads of a workgroup run one after the other.
HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
static unsigned long g_muls = 0;
#define ZKP_FR_COUNT_MUL (++g_muls)
#include "zkp_fr.hpp"
using namespace zkp::fr;
struct E { uint32_t w[NW]; };
static void put(const uint32_t* v, int n) { for (int i = n - 1; i >= 0; i--) std::printf("%08x", v[i]); std::printf("\n"); }
static void get(const char* hex, uint32_t* v, int n) {
    const size_t len = std::strlen(hex);
    for (int i = 0; i < n; i++) {
        char buf[9] = "00000000";
        for (int k = 0; k < 8; k++) {
            const long at = (long)len - 8 * (i + 1) + k;
            if (at >= 0) buf[k] = hex[at];
        }
        v[i] = (uint32_t)std::strtoul(buf, nullptr, 16);
    }
}
static E one() { constexpr Consts K = make_consts(); E e; for (int i = 0; i < NW; i++) e.w[i] = K.one[i]; return e; }
// oth[t] = the product of the totals of the other threads below na (any[t]: there is one); returns the total of all
static E others(const std::vector<E>& T, unsigned na, std::vector<E>& oth, std::vector<char>& any) {
    std::vector<E> P(T), Q(T);
    for (unsigned d = 1; d < na; d <<= 1) {
        std::vector<E> P0(P), Q0(Q);
        for (unsigned t = 0; t < na; t++) {
            if (t >= d) mont_mul(P[t].w, P[t].w, P0[t - d].w);
            if (t + d < na) mont_mul(Q[t].w, Q[t].w, Q0[t + d].w);
        }
    }
    for (unsigned t = 0; t < na; t++) {
        any[t] = 0;
        if (t > 0) { oth[t] = P[t - 1]; any[t] = 1; }
        if (t + 1 < na) {
            if (any[t]) mont_mul(oth[t].w, oth[t].w, Q[t + 1].w);
            else oth[t] = Q[t + 1];
            any[t] = 1;
        }
    }
    return P[na - 1];
}
static int load_run(const std::vector<E>& a, size_t first, InvRun& r) {
    const size_t n = a.size();
    const int m = first < n ? (n - first < (size_t)INV_RUN ? (int)(n - first) : INV_RUN) : 0;
    if (m > 0) std::memcpy(r.x0, a[first].w, 32);
    if (m > 1) std::memcpy(r.x1, a[first + 1].w, 32);
    if (m > 2) std::memcpy(r.x2, a[first + 2].w, 32);
    if (m > 3) std::memcpy(r.x3, a[first + 3].w, 32);
    return m;
}
static unsigned long g_pows = 0, g_pow_muls = 0;
static void invert_batch(const std::vector<E>& a, std::vector<E>& out) {
    constexpr Roots W = make_roots();
    const size_t n = a.size(), nb = (n + INV_BLOCK - 1) / INV_BLOCK;
    std::vector<E> tot(nb), pre(nb);
    for (size_t b = 0; b < nb; b++) {                                   // up
        const size_t base = b * INV_BLOCK, left = n - base;
        const unsigned na = left >= (size_t)INV_BLOCK ? INV_TPB : (unsigned)((left + INV_RUN - 1) / INV_RUN);
        std::vector<E> T(INV_TPB, one());
        for (unsigned t = 0; t < (unsigned)INV_TPB; t++) {
            InvRun r;
            std::memset(&r, 0, sizeof r);
            uint32_t zm;
            const int m = load_run(a, base + (size_t)t * INV_RUN, r);
            inv_run_prefix(r, T[t].w, &zm, m);
        }
        for (unsigned s = INV_TPB / 2; s >= 1; s >>= 1)
            for (unsigned t = 0; t < s; t++)
                if (t + s < na) mont_mul(T[t].w, T[t].w, T[t + s].w);
        tot[b] = T[0];
    }
    {                                                                   // mid
        const size_t run = (nb + INV_TPB - 1) / INV_TPB, na = (nb + run - 1) / run;
        std::vector<E> T(na, one()), oth(na);
        std::vector<char> any(na);
        for (size_t t = 0; t < na; t++) {
            const size_t lo = t * run, hi = nb - lo < run ? nb : lo + run;
            for (size_t j = lo; j < hi; j++) {
                if (j == lo) T[t] = tot[j];
                else mont_mul(T[t].w, T[t].w, tot[j].w);
                pre[j] = T[t];
            }
        }
        E g = others(T, (unsigned)na, oth, any);
        const unsigned long before = g_muls;
        mont_inv(g.w, g.w);
        g_pows++;
        g_pow_muls += g_muls - before;
        mont_mul(g.w, g.w, W.rinv);
        for (size_t t = 0; t < na; t++) {
            const size_t lo = t * run, hi = nb - lo < run ? nb : lo + run;
            E u = g;
            if (any[t]) mont_mul(u.w, oth[t].w, g.w);
            for (size_t j = hi; j-- > lo + 1;) {
                E o;
                mont_mul(o.w, u.w, pre[j - 1].w);
                mont_mul(u.w, u.w, tot[j].w);
                tot[j] = o;
            }
            tot[lo] = u;
        }
    }
    out.resize(n);
    for (size_t b = 0; b < nb; b++) {                                   // down
        const size_t base = b * INV_BLOCK, left = n - base;
        const unsigned na = left >= (size_t)INV_BLOCK ? INV_TPB : (unsigned)((left + INV_RUN - 1) / INV_RUN);
        std::vector<E> T(INV_TPB, one()), oth(INV_TPB);
        std::vector<char> any(INV_TPB);
        std::vector<InvRun> runs(INV_TPB);
        std::vector<uint32_t> zm(INV_TPB);
        std::vector<int> ms(INV_TPB);
        for (unsigned t = 0; t < (unsigned)INV_TPB; t++) {
            std::memset(&runs[t], 0, sizeof(InvRun));
            ms[t] = load_run(a, base + (size_t)t * INV_RUN, runs[t]);
            inv_run_prefix(runs[t], T[t].w, &zm[t], ms[t]);
        }
        others(T, na, oth, any);
        for (unsigned t = 0; t < na; t++) {
            E u = tot[b];
            if (any[t]) mont_mul(u.w, oth[t].w, tot[b].w);
            inv_run_back(runs[t], u.w, zm[t], ms[t]);
            const size_t first = base + (size_t)t * INV_RUN;
            if (ms[t] > 0) std::memcpy(out[first].w, runs[t].x0, 32);
            if (ms[t] > 1) std::memcpy(out[first + 1].w, runs[t].p1, 32);
            if (ms[t] > 2) std::memcpy(out[first + 2].w, runs[t].p2, 32);
            if (ms[t] > 3) std::memcpy(out[first + 3].w, runs[t].p3, 32);
        }
    }
}
int main() {
    char op[16], ha[160], hb[160];
    while (std::scanf("%15s %159s %159s", op, ha, hb) == 3) {
        uint32_t a[NW], b[NW], r[NW];
        if (!std::strcmp(op, "roots")) {
            constexpr Roots W = make_roots();
            for (int k = 0; k <= 32; k++) { from_mont(r, W.omega[k]); put(r, NW); }
            for (int k = 0; k <= 32; k++) { from_mont(r, W.inv_pow2[k]); put(r, NW); }
            put(W.rinv, NW);
            continue;
        }
        if (!std::strcmp(op, "invbatch")) {      // a: the number of elements, which follow one per line
            const unsigned long n = std::strtoul(ha, nullptr, 10);
            std::vector<E> in(n), out;
            for (unsigned long i = 0; i < n; i++) {
                if (std::scanf("%159s", ha) != 1) return 3;
                get(ha, in[i].w, NW);
            }
            g_muls = g_pows = g_pow_muls = 0;
            invert_batch(in, out);
            for (unsigned long i = 0; i < n; i++) put(out[i].w, NW);
            std::printf("%lu %lu\n", g_muls - g_pow_muls, g_pows);
            continue;
        }
        get(ha, a, NW); get(hb, b, NW);
        if (!std::strcmp(op, "pow")) zkp::fr::pow(r, a, b);
        else if (!std::strcmp(op, "montinv")) mont_inv(r, a);
        else return 2;
        put(r, NW);
    }
    return 0;
}
"""


def _compile(tmp_path, name, src, sanitize=("undefined",), opt="-O2"):
    f = tmp_path / (name + ".cpp")
    f.write_text(src)
    exe = str(tmp_path / name)
    flags = ["-fsanitize=" + ",".join(sanitize), "-fno-sanitize-recover=all"] if sanitize else []
    cc = subprocess.run(["g++", "-std=c++17", opt, "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", exe, str(f)],
                        capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def fr_exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("kzg_fr"), "kzg_fr_harness", HARNESS)


def _run(exe, text, timeout=900):
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split()


def _golden_operands():
    with open(os.path.join(ROOT, "tests", "golden", "fr_operands.json")) as f:
        g = json.load(f)
    vals = [int(g[k], 16) for k in ("largest", "fr_r", "fr_r2", "fr_r3")] + [int(v, 16) % R for v in g["from_u512"]]
    return sorted(set(v % R for v in vals))


def test_pow_against_python_pow(fr_exe):
    rng = random.Random(0x90F)
    bases = _golden_operands() + [0, 1, 2, R - 1, R - 2] + [rng.randrange(R) for _ in range(20)]
    exps = [0, 1, R - 2, R - 1, MONT - 1, 2, 1 << 255, (1 << 32) - 1, 1 << 32] + [rng.getrandbits(256) for _ in range(6)]
    pairs = [(a, e) for a in bases for e in exps]
    got = [int(x, 16) for x in _run(fr_exe, "".join("pow %x %x\n" % p for p in pairs))]
    assert got == [pow(a, e, R) for a, e in pairs]
    # the Montgomery-domain inverse the batched inversion takes once per call: R^2 / a, and 0 for 0
    vals = [0, 1, R - 1] + bases[:10]
    got = [int(x, 16) for x in _run(fr_exe, "".join("montinv %x 0\n" % a for a in vals))]
    assert got == [MONT * MONT * pow(a, R - 2, R) % R for a in vals]


def test_roots_of_unity_and_inverse_powers_of_two_are_derived_right(fr_exe):
    out = [int(x, 16) for x in _run(fr_exe, "roots 0 0\n")]
    omega, inv2, rinv = out[:33], out[33:66], out[66]
    assert omega[32] == pow(7, (R - 1) >> 32, R) and pow(omega[32], 1 << 31, R) == R - 1
    for k in (0, 1, 12, 20, 32):
        assert pow(omega[k], 1 << k, R) == 1 and (k == 0 or pow(omega[k], 1 << (k - 1), R) == R - 1), k
    for k in range(33):
        assert omega[k] == pow(omega[32], 1 << (32 - k), R) and inv2[k] * pow(2, k, R) % R == 1, k
    assert rinv * MONT % R == 1
    from zkvm_pairings_amd import synthetic
    assert [synthetic.fr_root_of_unity(k) for k in range(33)] == omega


def _inv(v):
    return pow(v, -1, R) if v else 0          # = pow(v, R - 2, R), and much faster on 10^5 values


def _invert_host(exe, vals):
    out = _run(exe, "invbatch %d 0\n" % len(vals) + "".join("%x\n" % v for v in vals))
    return [int(x, 16) for x in out[:len(vals)]], int(out[-2]), int(out[-1])


def _zero_patterns(n, rng):
    vals = [rng.randrange(1, R) for _ in range(n)]
    pats = [list(vals)]
    for idx in ([0], [n - 1], [n // 2], [0, 1], [n - 2, n - 1], list(range(max(0, n // 2 - 3), min(n, n // 2 + 3)))):
        p = list(vals)
        for i in idx:
            if 0 <= i < n:
                p[i] = 0
        pats.append(p)
    pats.append([0] * n)
    return pats


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9, 13, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000])
def test_host_replay_of_the_inversion_against_python_and_its_product_count(fr_exe, n):
    rng = random.Random(0x1A7 + n)
    for vals in _zero_patterns(n, rng):
        got, muls, pows = _invert_host(fr_exe, vals)
        assert got == [pow(v, R - 2, R) for v in vals]
        assert pows == 1 <= (n + 1023) // 1024 + 1 and muls <= 8 * n, (n, muls, pows)


def test_host_replay_with_a_middle_level_of_more_than_one_total_per_thread(fr_exe):
    """257 and 520 workgroups: the middle launch's threads own two and three totals; zeros across a workgroup boundary; 1, r - 1 and the
    golden operands among the values; a full workgroup costs 7.25 products per element"""
    rng = random.Random(0x1A8)
    for n in (256 * 1024 + 5, 520 * 1024):
        vals = [rng.randrange(1, R) for _ in range(n)]
        for i in range(1020, 1030):
            vals[i] = 0
        vals[0], vals[1], vals[n - 1] = 1, R - 1, 0
        for i, v in enumerate(_golden_operands()):
            vals[5000 + i] = v
        got, muls, pows = _invert_host(fr_exe, vals)
        assert got == [_inv(v) for v in vals]
        assert pows == 1 and muls <= 8 * n
        if n % 1024 == 0:
            assert 7.25 * n <= muls <= 7.26 * n, muls


def test_the_folded_equation_is_the_sum_of_the_per_opening_equations():
    """in the exponent (every point a multiple of a generator, e(G1, G2)^x written x): opening i holds iff c_i - y_i + z_i p_i - tau p_i = 0,
    and what the call tests, -(sum r_i c_i + sum t_i p_i - u) + tau sum r_i p_i with t_i = r_i z_i and u = sum r_i y_i, is
    -sum_i r_i (defect of opening i)"""
    rng = random.Random(0x7A6)
    for n in (1, 3, 7):
        tau = rng.randrange(1, R)
        c, z, y, p = ([rng.randrange(R) for _ in range(n)] for _ in range(4))
        r = [rng.getrandbits(64) + rng.getrandbits(64) * Z2 for _ in range(n)]
        assert all(0 < v < R for v in r)
        defect = [(c[i] - y[i] + z[i] * p[i] - tau * p[i]) % R for i in range(n)]
        t = [r[i] * z[i] % R for i in range(n)]
        u = sum(r[i] * y[i] for i in range(n)) % R
        lhs = (-(sum(r[i] * c[i] for i in range(n)) + sum(t[i] * p[i] for i in range(n)) - u) + tau * sum(r[i] * p[i] for i in range(n))) % R
        assert lhs == -sum(r[i] * defect[i] for i in range(n)) % R
        # an honest proof exponent makes the defect vanish
        p = [(c[i] - y[i]) * pow(tau - z[i], -1, R) % R for i in range(n)]
        assert all((c[i] - y[i] + z[i] * p[i] - tau * p[i]) % R == 0 for i in range(n))


@pytest.mark.parametrize("log2_n", [0, 1, 3])
@pytest.mark.parametrize("bitrev", [False, True])
def test_barycentric_model_agrees_with_horner_on_the_inverse_dft(log2_n, bitrev):
    from zkvm_pairings_amd import synthetic
    rng = random.Random(0xBA7 + log2_n)
    n = 1 << log2_n
    w = synthetic.fr_root_of_unity(log2_n)
    assert pow(w, n, R) == 1 and (n == 1 or pow(w, n // 2, R) == R - 1)
    coeff = [rng.randrange(R) for _ in range(n)]
    horner = lambda x: sum(c * pow(x, k, R) for k, c in enumerate(coeff)) % R
    natural = [horner(pow(w, i, R)) for i in range(n)]
    # the naive inverse DFT gives the coefficients back: the evaluations describe this polynomial
    ninv = pow(n, -1, R)
    assert [sum(natural[i] * pow(w, -i * k % n, R) for i in range(n)) * ninv % R for k in range(n)] == coeff
    evals = [natural[synthetic.bit_reverse(i, log2_n)] for i in range(n)] if bitrev else natural
    for z in [0, 1, R - 1, rng.randrange(R), rng.randrange(R)] + [pow(w, i, R) for i in (0, n // 2, n - 1)]:
        assert synthetic.barycentric_eval(evals, z, log2_n, bitrev) == horner(z), z


LAYOUT = r"""
#include <cstdio>
#include <cstddef>
#include "zkp_pairings.h"
#define V(x) std::printf("vk.%s %zu\n", #x, offsetof(zkp_kzg_vk, x));
#define B(x) std::printf("b.%s %zu\n", #x, offsetof(zkp_kzg_batch, x));
int main() {
    V(g1) V(g2) V(tau_g2)
    B(n) B(c) B(inf_c) B(proof) B(inf_proof) B(z) B(y)
    std::printf("sizeof_vk %zu\nsizeof_b %zu\npoints %d\nvk %d\nbitrev %d\n", sizeof(zkp_kzg_vk), sizeof(zkp_kzg_batch), ZKP_KZG_POINTS_CHECKED, ZKP_KZG_VK_CHECKED,
                ZKP_FR_EVAL_BITREV);
    return 0;
}
"""


def test_struct_layouts_and_flags_agree_in_header_ctypes_and_rust(tmp_path):
    from zkvm_pairings_amd import _lib
    exe = _compile(tmp_path, "kzg_layout", LAYOUT, sanitize=None, opt="-O1")
    lines = [line.split() for line in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split("\n") if line]
    rows = {r[0]: r[1:] for r in lines}
    assert [n for n, _ in _lib.KzgVk._fields_] == VK_FIELDS and [n for n, _ in _lib.KzgBatch._fields_] == BATCH_FIELDS
    for name in VK_FIELDS:
        assert getattr(_lib.KzgVk, name).offset == int(rows["vk." + name][0]), name
    for name in BATCH_FIELDS:
        assert getattr(_lib.KzgBatch, name).offset == int(rows["b." + name][0]), name
    assert ctypes.sizeof(_lib.KzgVk) == int(rows["sizeof_vk"][0]) and ctypes.sizeof(_lib.KzgBatch) == int(rows["sizeof_b"][0])
    assert _lib.KZG_POINTS_CHECKED == int(rows["points"][0]) == 1 and _lib.KZG_VK_CHECKED == int(rows["vk"][0]) == 2
    assert _lib.FR_EVAL_BITREV == int(rows["bitrev"][0]) == 1
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        rust = f.read()
    for struct, names, sizes in (("zkp_kzg_vk", VK_FIELDS, ()), ("zkp_kzg_batch", BATCH_FIELDS, ("n",))):
        body = re.search(r"#\[repr\(C\)\]\s*(?:#\[[^\]]*\]\s*)*pub struct %s \{(.*?)\}" % struct, rust, re.S).group(1)
        fields = re.findall(r"pub (\w+):\s*([^,]+),", body)
        assert [n for n, _ in fields] == names
        for n, t in fields:
            assert t.strip() == ("usize" if n in sizes else "*const c_void"), (n, t)
    for name, v in (("ZKP_KZG_POINTS_CHECKED", 1), ("ZKP_KZG_VK_CHECKED", 2), ("ZKP_FR_EVAL_BITREV", 1)):
        assert re.search(r"pub const %s: c_int = %d;" % (name, v), rust), name


PLAN_CHECK = r"""
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "zkp_groth16_plan.hpp"
#include "zkp_kzg_plan.hpp"
using namespace zkp::kzg;
static int fails = 0;
#define REQ(x) do { if (!(x)) { std::printf("FAIL %s at %zu %zu\n", #x, (size_t)A, (size_t)B); fails++; return; } } while (0)
typedef unsigned __int128 u128;
static void check_inv(size_t n) {
    const size_t A = n, B = 0;
    if (inv_args_bad(n) || !n) return;
    const InvPlan p = inv_plan(n);
    REQ((u128)p.blocks * INV_BLOCK >= n && (u128)(p.blocks - 1) * INV_BLOCK < n && p.blocks <= 0x7fffffff);
    REQ(p.mid_run >= 1 && p.mid_threads >= 1 && p.mid_threads <= INV_TPB && (u128)p.mid_threads * p.mid_run >= p.blocks &&
        (u128)(p.mid_threads - 1) * p.mid_run < p.blocks);
    REQ(p.tot + p.blocks * 32 <= p.pre && p.pre + p.blocks * 32 <= p.total && p.pre % 256 == 0 && p.total <= p.blocks * 64 + 512);
}
static void check_eval(size_t n_poly, unsigned k, int flags) {
    const size_t A = n_poly, B = k;
    if (eval_args_bad(n_poly, k, flags) || !n_poly) return;
    const EvalLayout L = eval_layout(n_poly, k);
    const size_t evals = n_poly << k;
    REQ(evals <= EVAL_MAX_TOTAL && evals >> k == n_poly);
    REQ(L.inv.total <= L.den && L.den % 256 == 0 && L.den + evals * 32 <= L.total);
    REQ(L.total <= evals * 32 + L.inv.total + 256 && L.inv.total <= evals / 16 + 1024);      // 32 B per evaluation, 64 B per 1024
    REQ(L.tp_log2 == (k < 8 ? k : 8) && (u128)L.sum_blocks * (INV_TPB >> L.tp_log2) >= n_poly && (u128)(L.sum_blocks - 1) * (INV_TPB >> L.tp_log2) < n_poly);
    REQ(L.sum_blocks <= 0x7fffffff && domain_bytes(k) == ((size_t)32 << k));
}
static void check_kzg(size_t n, int flags) {
    const size_t A = n, B = (size_t)flags;
    if (args_bad(n, flags) || !n) return;
    REQ(!zkp::g16::fold_args_bad(n, 1));
    const zkp::g16::FoldPlan fp = zkp::g16::fold_plan(n, 1);
    const Layout L = make_layout(n, flags, fp.part_bytes, fp.sum_bytes);
    REQ(L.n_status == ((flags & POINTS_CHECKED) ? 0 : 2 * n) + ((flags & VK_CHECKED) ? 0 : 3));
    REQ(L.flag + 8 <= L.st && L.st + L.n_status <= L.ms && L.ms + 2 * (2 * n + 1) * 32 <= L.mp && L.mp + (2 * n + 1) * 96 <= L.minf && L.minf + 2 * n + 1 <= L.part);
    REQ(L.part + fp.part_bytes <= L.sum && L.sum + fp.sum_bytes <= L.u && L.u + 32 <= L.mg1 && L.mg1 + 2 * 96 <= L.minf1 && L.minf1 + 2 <= L.mg2);
    REQ(L.mg2 + 2 * 192 <= L.ml && L.ml + ML_RECORDS * 576 <= L.total);
    REQ(L.ms % 256 == 0 && L.mp % 256 == 0 && L.part % 256 == 0 && L.u % 256 == 0 && L.ml % 256 == 0);
    const u128 need = (u128)8 + L.n_status + (u128)(2 * n + 1) * (64 + 96 + 1) + fp.part_bytes + fp.sum_bytes + 32 + 2 * 96 + 2 + 2 * 192 + ML_RECORDS * 576;
    REQ((u128)L.total >= need && (u128)L.total <= need + 12 * 256);
    REQ(2 * n + 1 <= ((size_t)1 << 24) && (n == MAX_OPENINGS) == (2 * (2 * n + 1) > ((size_t)1 << 24)));   // one shared-bases MSM call, but for the largest batch
}
int main() {
    for (size_t n : {(size_t)1, (size_t)2, (size_t)4, (size_t)5, (size_t)1023, (size_t)1024, (size_t)1025, (size_t)5000, (size_t)65539, (size_t)262143, (size_t)262144,
                     (size_t)262145, (size_t)1 << 24, ((size_t)1 << 28) + 1, INV_MAX - 1, INV_MAX, INV_MAX + 1})
        check_inv(n);
    for (unsigned k = 0; k <= EVAL_MAX_LOG2 + 1; k++)
        for (size_t n_poly : {(size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)63, (size_t)64, (size_t)65, (size_t)255, (size_t)256, (size_t)257, (size_t)4096,
                              EVAL_MAX_TOTAL >> (k < 27 ? k : 26), (EVAL_MAX_TOTAL >> (k < 27 ? k : 26)) + 1})
            for (int flags = 0; flags < 2; flags++) check_eval(n_poly, k, flags);
    for (size_t n : {(size_t)1, (size_t)2, (size_t)5, (size_t)127, (size_t)255, (size_t)256, (size_t)257, (size_t)1000, (size_t)1 << 10, (size_t)1 << 18, MAX_OPENINGS - 1,
                     MAX_OPENINGS, MAX_OPENINGS + 1})
        for (int flags = 0; flags < 4; flags++) check_kzg(n, flags);
    const bool lim = !inv_args_bad(0) && !inv_args_bad(INV_MAX) && inv_args_bad(INV_MAX + 1) && inv_args_bad(SIZE_MAX) &&
                     !eval_args_bad(0, 0, 0) && !eval_args_bad(0, 20, 1) && eval_args_bad(0, 21, 0) && eval_args_bad(1, 21, 0) && eval_args_bad(1, 64, 0) &&
                     eval_args_bad(1, 0xffffffffu, 0) && !eval_args_bad((size_t)1 << 26, 0, 0) && eval_args_bad(((size_t)1 << 26) + 1, 0, 0) &&
                     !eval_args_bad(64, 20, 0) && eval_args_bad(65, 20, 0) && !eval_args_bad((size_t)1 << 14, 12, 1) && eval_args_bad(((size_t)1 << 14) + 1, 12, 1) &&
                     eval_args_bad(1, 1, 2) && eval_args_bad(1, 1, -1) && eval_args_bad(SIZE_MAX, 1, 0) &&
                     !args_bad(0, 0) && !args_bad(MAX_OPENINGS, 3) && args_bad(MAX_OPENINGS + 1, 0) && args_bad(SIZE_MAX, 0) && args_bad(1, 4) && args_bad(1, -1) &&
                     args_bad(0, 4);
    if (!lim) { std::printf("FAIL the ABI limits\n"); fails++; }
    if (fails) return 1;
    std::printf("kzg plan_check ok\n");
    return 0;
}
"""


def test_planner_under_asan_and_ubsan_at_the_abi_maxima(tmp_path):
    exe = _compile(tmp_path, "kzg_plan_check", PLAN_CHECK, sanitize=("address", "undefined"), opt="-O1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "kzg plan_check ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    for src in ("zkp_kzg.hip", "zkp_pairings.hip"):
        with open(os.path.join(CSRC, src)) as f:
            assert '#include "zkp_kzg_plan.hpp"' in f.read()


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_frinv_" in n or "k_freval_" in n or "k_kzg_" in n}
    # inversion: up, mid, down; evaluation: domain, den, sum; verifier: init, status, scalars, g2, place, finish
    assert len(new) == 3 + 3 + 6, sorted(new)
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)
    (down,) = [v for n, v in new.items() if "k_frinv_down" in n]
    assert down["vgpr"] <= 168 and down["lds"] == 2 * 8 * 256 * 4, down              # three waves per SIMD; the two scans' LDS


def test_new_symbols_are_exported_and_refuse_a_null_context():
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.zkp_abi_version() == 4
    one = ctypes.c_int(0)
    vk, b = _lib.KzgVk(), _lib.KzgBatch(n=0)
    assert lib.zkp_kzg_verify_batch(None, ctypes.byref(vk), ctypes.byref(b), None, 0, ctypes.byref(one)) == -1
    assert lib.zkp_kzg_verify_batch_dev(None, ctypes.byref(vk), ctypes.byref(b), None, 0, None, None) == -1
    assert lib.zkp_fr_invert_batch(None, None, 0, None) == -1 and lib.zkp_fr_invert_batch_dev(None, None, 0, None, None) == -1
    assert lib.zkp_fr_eval_batch(None, None, None, 0, 0, 0, None) == -1 and lib.zkp_fr_eval_batch_dev(None, None, None, 0, 0, 0, None, None) == -1


def test_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import synthetic
    for name in ("fr_invert", "fr_eval", "kzg_verify_batch"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("KzgSetup", "kzg_verify_batch", "kzg_verify_each", "kzg_verify_blob_batch"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.Fr.invert_batch) and callable(z.Fr.evaluate) and callable(synthetic.kzg_instance) and callable(synthetic.kzg_blob_instance)
    with open(os.path.join(ROOT, "include", "zkp_pairings.h")) as f:
        h = f.read()
    assert h.count("added under ABI version 4") >= 2 and re.search(r"\* +zkp_fr_invert_batch .*src/fr\.rs:\d+", h)
