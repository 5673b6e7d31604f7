"""CPU gate for the batch check by random linear combination: a Python model of r = a + b z^2 against the oracle ((beta x, -y) is [z^2]P
on G1, the map (a, b) -> a + b z^2 is injective below r) and against the planner's own scalar function, the layouts of zkp_rlc_batch in
the header, ctypes and Rust agree, the RLC planner (csrc/zkp_rlc_plan.hpp) holds at the ABI maxima under ASan and UBSan, and the new
kernels neither spill nor use scratch in the built code object."""
import os
import re
import subprocess

import numpy as np
import pytest

import bls12_381_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
P, R = bm.P, bm.R_ORDER
Z2 = bm.BLS_X ** 2
M64 = (1 << 64) - 1
EDGE = [0, 1, 2, M64 - 1, M64]
FIELDS = ["n_checks", "k", "g1", "g2", "inf1", "inf2", "s2", "col_g1", "col_inf1", "fixed_g2", "fixed_inf2", "s1", "col_g2", "col_inf2",
          "fixed_g1", "fixed_inf1"]


def _compile(tmp_path, name, src, sanitize=False):
    f = tmp_path / (name + ".cpp")
    f.write_text(src)
    exe = str(tmp_path / name)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", exe,
                         str(f)], capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def test_z2_is_the_planner_constant_and_the_scalars_are_injective_below_r():
    assert Z2 == 0xAC45A4010001A402_0000000100000000
    vals = {(a, b): a + b * Z2 for a in EDGE for b in EDGE}
    assert len(set(vals.values())) == len(vals)                         # a < 2^64 < z^2: (a, b) is the quotient / remainder of r by z^2
    assert max(vals.values()) < R and max(vals.values()) < 1 << 192
    assert all(v == 0 for (a, b), v in vals.items() if a == 0 and b == 0) and sorted(vals.values())[1] > 0


def test_beta_x_minus_y_is_z2_times_p_on_g1():
    import oracle_lib as o
    g = o.g1_generator()
    for k in (1, 2, 12345, R - 1, 0xDEADBEEF << 100):
        p, inf = o.g1_mul(g, k)
        assert not inf
        want, wi = o.g1_mul(p, Z2)
        x, y = o.from_limbs(p[:6]), o.from_limbs(p[6:])
        phi = np.concatenate([o.to_limbs(x * bm.BETA % P), o.to_limbs((P - y) % P)])
        assert wi == 0 and np.array_equal(want, phi), k
        # and so [a]P + [b]phi(P) = [a + b z^2]P
        a, b = 0x1234567890ABCDEF, M64
        s, si = o.g1_add(*o.g1_mul(p, a), *o.g1_mul(phi, b))
        assert np.array_equal(s, o.g1_mul(p, (a + b * Z2) % R)[0]) and si == 0


SCALAR = r"""
#include <cstdio>
#include <cinttypes>
#include "zkp_rlc_plan.hpp"
int main() {
    unsigned long long a, b;
    while (std::scanf("%llu %llu", &a, &b) == 2) {
        uint64_t r[4];
        zkp::rlc::scalar(a, b, r);
        std::printf("%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "\n", r[3], r[2], r[1], r[0]);
    }
    return 0;
}
"""


def test_planner_scalar_function_matches_the_model(tmp_path):
    import random
    exe = _compile(tmp_path, "rlc_scalar", SCALAR, sanitize=True)
    rng = random.Random(0x5CA1)
    pairs = [(a, b) for a in EDGE for b in EDGE] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(500)]
    out = subprocess.run([exe], input="".join("%d %d\n" % p for p in pairs), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [int(x, 16) for x in out.stdout.split()]
    assert got == [a + b * Z2 for a, b in pairs]


LAYOUT = r"""
#include <cstdio>
#include <cstddef>
#include "zkp_pairings.h"
#define F(x) std::printf("%s %zu\n", #x, offsetof(zkp_rlc_batch, x));
int main() {
    F(n_checks) F(k) F(g1) F(g2) F(inf1) F(inf2) F(s2) F(col_g1) F(col_inf1) F(fixed_g2) F(fixed_inf2) F(s1) F(col_g2) F(col_inf2) F(fixed_g1)
    F(fixed_inf1)
    std::printf("sizeof %zu\nflag %d\n", sizeof(zkp_rlc_batch), ZKP_RLC_POINTS_CHECKED);
    return 0;
}
"""


def test_rlc_batch_layout_agrees_in_header_ctypes_and_rust(tmp_path):
    from zkvm_pairings_amd import _lib
    exe = _compile(tmp_path, "rlc_layout", LAYOUT)
    rows = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split("\n") if line)
    c_order = [f for f in FIELDS]
    assert [n for n, _ in _lib.RlcBatch._fields_] == c_order
    for name in FIELDS:
        assert getattr(_lib.RlcBatch, name).offset == int(rows[name]), name
    assert __import__("ctypes").sizeof(_lib.RlcBatch) == int(rows["sizeof"])
    assert _lib.RLC_POINTS_CHECKED == int(rows["flag"])
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        rust = f.read()
    body = re.search(r"#\[repr\(C\)\]\s*(?:#\[[^\]]*\]\s*)*pub struct zkp_rlc_batch \{(.*?)\}", rust, re.S).group(1)
    fields = re.findall(r"pub (\w+):\s*([^,]+),", body)
    assert [n for n, _ in fields] == FIELDS
    for n, t in fields:
        assert t.strip() == ("usize" if n in ("n_checks", "k", "s1", "s2") else "*const c_void"), (n, t)
    assert re.search(r"pub const ZKP_RLC_POINTS_CHECKED: c_int = %s;" % rows["flag"], rust)


PLAN_CHECK = r"""
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "zkp_rlc_plan.hpp"
using namespace zkp::rlc;
static int fails = 0;
#define REQ(x) do { if (!(x)) { std::printf("FAIL %s n=%zu k=%zu s1=%zu s2=%zu\n", #x, n, k, s1, s2); fails++; return; } } while (0)
typedef unsigned __int128 u128;
static void check(size_t n, size_t k, size_t s1, size_t s2, bool chk) {
    if (args_bad(n, k, s1, s2) || !n) return;
    const Layout L = make_layout(n, k, s1, s2, chk);
    const size_t smax = s1 > s2 ? s1 : s2;
    REQ(L.cols <= smax && (u128)L.cols * n <= MAX_COL_TERMS && (smax == 0 || L.cols >= 1));
    REQ(L.n_status == (chk ? (u128)2 * n * k + (u128)(n + 1) * (s1 + s2) : 0));
    // every region at least as large as what the driver writes into it, in order, and no size wrapped
    const u128 need = (u128)8 + L.n_status + (u128)L.cols * n * 32 + (u128)n * k * 97 + (u128)n * s2 * 97 + (u128)n * s1 * 193 +
                      (u128)(s1 + s2) * (96 + 192 + 2) + ML_RECORDS * 576;
    REQ((u128)L.total >= need && (u128)L.total <= need + 14 * 256);
    REQ(L.flag < L.st || L.n_status == 0);
    REQ(L.sc + L.cols * n * 32 <= L.sg1 && L.sg1 + n * k * 96 <= L.sinf && L.sinf + n * k <= L.tg1 && L.tg1 + n * s2 * 96 <= L.tinf1);
    REQ(L.tinf1 + n * s2 <= L.tg2 && L.tg2 + n * s1 * 192 <= L.tinf2 && L.tinf2 + n * s1 <= L.mg1 && L.mg1 + (s1 + s2) * 96 <= L.mg2);
    REQ(L.mg2 + (s1 + s2) * 192 <= L.minf1 && L.minf1 + s1 + s2 <= L.minf2 && L.minf2 + s1 + s2 <= L.ml && L.ml + ML_RECORDS * 576 <= L.total);
    REQ(n * k <= MAX_PAIRS && (s1 + s2 == 0 || n <= MAX_COL_TERMS));
}
int main() {
    for (size_t n : {(size_t)1, (size_t)2, (size_t)7, (size_t)1000, (size_t)1 << 14, (size_t)1 << 18, MAX_COL_TERMS - 1, MAX_COL_TERMS,
                     MAX_COL_TERMS + 1, (size_t)1 << 28, MAX_PAIRS})
        for (size_t k : {(size_t)0, (size_t)1, (size_t)3, (size_t)8, (size_t)127, MAX_COLS})
            for (size_t s1 : {(size_t)0, (size_t)1, (size_t)3, MAX_COLS})
                for (size_t s2 : {(size_t)0, (size_t)1, (size_t)3, (size_t)1000, MAX_COLS})
                    for (int chk = 0; chk < 2; chk++) check(n, k, s1, s2, chk != 0);
    // the limits themselves
    const bool lim = !args_bad(0, 0, 0, 0) && args_bad(1, 0, 0, 0) && !args_bad(1, 0, 1, 0) && !args_bad(MAX_PAIRS, 1, 0, 0) && args_bad(MAX_PAIRS + 1, 1, 0, 0) &&
                     args_bad(1, MAX_COLS + 1, 0, 0) && args_bad(1, 1, MAX_COLS + 1, 0) && args_bad(1, 1, 0, MAX_COLS + 1) && !args_bad(MAX_COL_TERMS, 1, 1, 1) &&
                     args_bad(MAX_COL_TERMS + 1, 1, 1, 0) && !args_bad(MAX_COL_TERMS + 1, 1, 0, 0) && args_bad((size_t)1 << 20, (size_t)1 << 12, 0, 0) &&
                     args_bad(SIZE_MAX, 1, 0, 0) && args_bad(SIZE_MAX, SIZE_MAX, SIZE_MAX, SIZE_MAX);
    if (!lim) { std::printf("FAIL the ABI limits\n"); fails++; }
    for (size_t n : {(size_t)1 << 14, (size_t)1 << 18}) {
        const Layout g = make_layout(n, 1, 0, 3, true), b = make_layout(n, 1, 1, 0, true), f = make_layout(n, 3, 0, 0, true);
        std::printf("bytes per check at n=%zu: groth16 %.0f bls %.0f free3 %.0f\n", n, (double)g.total / n, (double)b.total / n, (double)f.total / n);
    }
    if (fails) return 1;
    std::printf("rlc plan_check ok\n");
    return 0;
}
"""


def test_rlc_planner_under_asan_and_ubsan_at_the_abi_maxima(tmp_path):
    exe = _compile(tmp_path, "rlc_plan_check", PLAN_CHECK, sanitize=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "rlc plan_check ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    with open(os.path.join(CSRC, "zkp_rlc.hip")) as f:
        assert '#include "zkp_rlc_plan.hpp"' in f.read()


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_do_not_spill():
    from test_msm_cpu import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_g1_mul_endo28" in n or "k_rlc_" in n}
    assert len(new) == 1 + 5, sorted(new)                      # the scaling kernel; init, fold, scalars, transpose, finish
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)


def test_new_symbols_are_exported_and_refuse_a_null_context():
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    for n in ("zkp_g1_mul_endo_batch", "zkp_g1_mul_endo_batch_dev", "zkp_pairing_check_batch_rlc", "zkp_pairing_check_batch_rlc_dev"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    one = __import__("ctypes").c_int(0)
    b = _lib.RlcBatch(n_checks=0)
    assert lib.zkp_pairing_check_batch_rlc(None, __import__("ctypes").byref(b), None, 0, __import__("ctypes").byref(one)) == -1
    assert lib.zkp_g1_mul_endo_batch(None, None, None, None, 0, None, None) == -1
