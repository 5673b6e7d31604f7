"""CPU gate for the batched Groth16 verifier: the planner (csrc/zkp_groth16_plan.hpp) holds at the ABI maxima under ASan and UBSan, the
layouts of zkp_groth16_vk / zkp_groth16_batch and the flags agree in the header, ctypes and Rust, the new kernels neither spill nor use
scratch in the built code object, the new symbols are exported and refuse a null context, and the combination the verifier tests is the
product of the per-proof equations (a Python model in the exponent)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
VK_FIELDS = ["alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "n_inputs", "ic"]
BATCH_FIELDS = ["n", "a", "inf_a", "b", "inf_b", "c", "inf_c", "inputs"]
NEW = ["zkp_fr_op_batch", "zkp_fr_op_batch_dev", "zkp_fr_from_wide_batch", "zkp_fr_from_wide_batch_dev", "zkp_fr_fold_batch", "zkp_fr_fold_batch_dev",
       "zkp_groth16_verify_batch", "zkp_groth16_verify_batch_dev"]


def _compile(tmp_path, name, src, sanitize=False):
    f = tmp_path / (name + ".cpp")
    f.write_text(src)
    exe = str(tmp_path / name)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", exe,
                         str(f)], capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def test_the_folded_equation_is_the_product_of_the_per_proof_equations():
    """in the exponent (every point a multiple of a generator, e(G1, G2)^x written x): proof c holds iff s t = a b + g vk_x + d c', and
    sum_c r_c (s t) - d sum_c r_c c' - g sum_i s_i k_i - s_0 a b == sum_c r_c (per-proof defect) for the s_i the fold forms"""
    rng = random.Random(0x616)
    for n, l in ((1, 0), (3, 1), (7, 5)):
        a, b, g, d = (rng.randrange(1, R) for _ in range(4))
        k = [rng.randrange(R) for _ in range(l + 1)]
        x = [[rng.randrange(R) for _ in range(l)] for _ in range(n)]
        s, t, cc = ([rng.randrange(R) for _ in range(n)] for _ in range(3))
        r = [rng.getrandbits(64) + rng.getrandbits(64) * 0xAC45A4010001A4020000000100000000 for _ in range(n)]
        defect = [(s[c] * t[c] - a * b - g * (k[0] + sum(x[c][i] * k[i + 1] for i in range(l))) - d * cc[c]) % R for c in range(n)]
        s_fold = [sum(r) % R] + [sum(r[c] * x[c][i] for c in range(n)) % R for i in range(l)]
        lhs = (sum(r[c] * s[c] * t[c] for c in range(n)) - d * sum(r[c] * cc[c] for c in range(n)) - g * sum(s_fold[i] * k[i] for i in range(l + 1)) -
               s_fold[0] * a * b) % R
        assert lhs == sum(r[c] * defect[c] for c in range(n)) % R


LAYOUT = r"""
#include <cstdio>
#include <cstddef>
#include "zkp_pairings.h"
#define V(x) std::printf("vk.%s %zu\n", #x, offsetof(zkp_groth16_vk, x));
#define B(x) std::printf("b.%s %zu\n", #x, offsetof(zkp_groth16_batch, x));
int main() {
    V(alpha_g1) V(beta_g2) V(gamma_g2) V(delta_g2) V(n_inputs) V(ic)
    B(n) B(a) B(inf_a) B(b) B(inf_b) B(c) B(inf_c) B(inputs)
    std::printf("sizeof_vk %zu\nsizeof_b %zu\npoints %d\nvk %d\n", sizeof(zkp_groth16_vk), sizeof(zkp_groth16_batch), ZKP_GROTH16_POINTS_CHECKED,
                ZKP_GROTH16_VK_CHECKED);
    std::printf("ops %d %d %d %d %d %d\n", ZKP_FR_MUL, ZKP_FR_ADD, ZKP_FR_SUB, ZKP_FR_NEG, ZKP_FR_SQUARE, ZKP_FR_INVERT);
    return 0;
}
"""


def test_struct_layouts_and_flags_agree_in_header_ctypes_and_rust(tmp_path):
    from zkvm_pairings_amd import _lib
    from zkvm_pairings_amd.engine import PairingEngine
    exe = _compile(tmp_path, "g16_layout", LAYOUT)
    lines = [line.split() for line in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split("\n") if line]
    rows = {r[0]: r[1:] for r in lines}
    assert [n for n, _ in _lib.Groth16Vk._fields_] == VK_FIELDS and [n for n, _ in _lib.Groth16Batch._fields_] == BATCH_FIELDS
    for name in VK_FIELDS:
        assert getattr(_lib.Groth16Vk, name).offset == int(rows["vk." + name][0]), name
    for name in BATCH_FIELDS:
        assert getattr(_lib.Groth16Batch, name).offset == int(rows["b." + name][0]), name
    assert ctypes.sizeof(_lib.Groth16Vk) == int(rows["sizeof_vk"][0]) and ctypes.sizeof(_lib.Groth16Batch) == int(rows["sizeof_b"][0])
    assert _lib.GROTH16_POINTS_CHECKED == int(rows["points"][0]) == 1 and _lib.GROTH16_VK_CHECKED == int(rows["vk"][0]) == 2
    assert [int(v) for v in rows["ops"]] == [0, 1, 2, 3, 4, 5]
    assert [PairingEngine.FR_OPS[k] for k in ("mul", "add", "sub", "neg", "square", "invert")] == [0, 1, 2, 3, 4, 5]
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        rust = f.read()
    for struct, names, sizes in (("zkp_groth16_vk", VK_FIELDS, ("n_inputs",)), ("zkp_groth16_batch", BATCH_FIELDS, ("n",))):
        body = re.search(r"#\[repr\(C\)\]\s*(?:#\[[^\]]*\]\s*)*pub struct %s \{(.*?)\}" % struct, rust, re.S).group(1)
        fields = re.findall(r"pub (\w+):\s*([^,]+),", body)
        assert [n for n, _ in fields] == names
        for n, t in fields:
            assert t.strip() == ("usize" if n in sizes else "*const c_void"), (n, t)
    assert re.search(r"pub const ZKP_GROTH16_POINTS_CHECKED: c_int = 1;", rust) and re.search(r"pub const ZKP_GROTH16_VK_CHECKED: c_int = 2;", rust)
    for i, name in enumerate(("MUL", "ADD", "SUB", "NEG", "SQUARE", "INVERT")):
        assert re.search(r"pub const ZKP_FR_%s: c_int = %d;" % (name, i), rust)


def test_header_says_the_symbols_came_under_version_4_and_cites_the_reference():
    with open(os.path.join(ROOT, "include", "zkp_pairings.h")) as f:
        h = f.read()
    assert "added under ABI version 4" in h
    for row in ("zkp_fr_op_batch", "zkp_fr_from_wide_batch"):
        assert re.search(r"\* +%s .*src/fr\.rs:\d+" % row, h), row


PLAN_CHECK = r"""
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "zkp_groth16_plan.hpp"
using namespace zkp::g16;
static int fails = 0;
#define REQ(x) do { if (!(x)) { std::printf("FAIL %s n=%zu l=%zu flags=%d\n", #x, n, l, flags); fails++; return; } } while (0)
typedef unsigned __int128 u128;
static void check(size_t n, size_t l, int flags) {
    if (args_bad(n, l, flags) || !n) return;
    const FoldPlan p = fold_plan(n, l);
    // the grid: tw a power of two that divides the workgroup, every i and every row covered, no more partial sums than rows
    REQ(p.tw >= 1 && p.tw <= FOLD_MAX_TW && (p.tw & (p.tw - 1)) == 0 && p.rows * p.tw == FOLD_TPB);
    REQ((u128)p.tiles * p.tw >= l && (l == 0 || (u128)(p.tiles - 1) * p.tw < l) && (l == 0) == (p.tiles == 0));
    REQ((l == 0) == (p.parts == 0) && (u128)p.parts * p.rows < (u128)n + p.rows && p.sum_parts >= 1 && (u128)p.sum_parts * FOLD_TPB < (u128)n + FOLD_TPB);
    REQ((u128)p.tiles * p.parts <= (u128)FOLD_BLOCKS + p.tiles && p.parts <= 65535 && p.sum_parts <= 65535 && p.tiles <= FOLD_BLOCKS);
    REQ((u128)p.part_bytes == (u128)p.parts * l * ACC_BYTES && p.sum_bytes == (size_t)p.sum_parts * ACC_BYTES);
    REQ(p.part_bytes <= (size_t)(FOLD_BLOCKS + FOLD_MAX_TW) * FOLD_MAX_TW * ACC_BYTES + MAX_INPUTS * ACC_BYTES);
    const FoldLayout F = fold_layout(p);
    REQ(F.part + p.part_bytes <= F.sum && F.sum + p.sum_bytes <= F.total);
    const Layout L = make_layout(n, l, flags);
    REQ(L.n_status == ((flags & POINTS_CHECKED) ? 0 : (u128)3 * n) + ((flags & VK_CHECKED) ? 0 : (u128)l + 5));
    // every region at least as large as what the driver writes into it, in order, and no size wrapped
    const u128 need = (u128)8 + L.n_status + (u128)n * (32 + 96 + 1) + p.part_bytes + p.sum_bytes + (u128)2 * (l + 1) * (32 + 96) + 3 * 96 + 3 + 3 * 192 +
                      ML_RECORDS * 576;
    REQ((u128)L.total >= need && (u128)L.total <= need + 13 * 256);
    REQ(L.flag + 8 <= L.st && L.st + L.n_status <= L.sc && L.sc + n * 32 <= L.sg1 && L.sg1 + n * 96 <= L.sinf && L.sinf + n <= L.part);
    REQ(L.part + p.part_bytes <= L.sum && L.sum + p.sum_bytes <= L.ms && L.ms + 2 * (l + 1) * 32 <= L.mp && L.mp + 2 * (l + 1) * 96 <= L.mg1);
    REQ(L.mg1 + 3 * 96 <= L.minf1 && L.minf1 + 3 <= L.mg2 && L.mg2 + 3 * 192 <= L.ml && L.ml + ML_RECORDS * 576 <= L.total);
    REQ(L.sc % 256 == 0 && L.part % 256 == 0 && L.ms % 256 == 0 && L.mp % 256 == 0 && L.ml % 256 == 0);
}
int main() {
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)4, (size_t)5, (size_t)63, (size_t)64, (size_t)65, (size_t)255, (size_t)256, (size_t)257, (size_t)1000,
                     (size_t)1 << 14, (size_t)1 << 18, ((size_t)1 << 18) + 1, (size_t)32768, (size_t)32769, MAX_PROOFS - 1, MAX_PROOFS, MAX_PROOFS + 1})
        for (size_t l : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)8, (size_t)63, (size_t)64, (size_t)65, (size_t)127, (size_t)128, (size_t)1000, (size_t)1023,
                         (size_t)1024, (size_t)1025, (size_t)65534, MAX_INPUTS, MAX_INPUTS + 1})
            for (int flags = 0; flags < 4; flags++) check(n, l, flags);
    // the limits themselves
    const bool lim = !args_bad(0, 0, 0) && !args_bad(MAX_PROOFS, 0, 3) && args_bad(MAX_PROOFS + 1, 0, 0) && !args_bad(1, MAX_INPUTS, 0) && args_bad(1, MAX_INPUTS + 1, 0) &&
                     !args_bad(MAX_PROOFS, 127, 0) && args_bad(MAX_PROOFS, 128, 0) && !args_bad(32768, MAX_INPUTS, 0) && args_bad(32769, MAX_INPUTS, 0) &&
                     args_bad(1, 1, 4) && args_bad(1, 1, -1) && args_bad(SIZE_MAX, SIZE_MAX, 0) && args_bad(SIZE_MAX, 1, 0) && !args_bad(0, MAX_INPUTS, 0) &&
                     fold_args_bad(MAX_PROOFS + 1, 0) && !fold_args_bad(MAX_PROOFS, 127) && fold_args_bad(MAX_PROOFS, 128);
    if (!lim) { std::printf("FAIL the ABI limits\n"); fails++; }
    for (size_t n : {(size_t)1 << 14, (size_t)1 << 18})
        for (size_t l : {(size_t)1, (size_t)8, (size_t)64}) {
            const Layout g = make_layout(n, l, 0);
            std::printf("bytes per proof at n=%zu l=%zu: %.1f\n", n, l, (double)g.total / n);
        }
    if (fails) return 1;
    std::printf("groth16 plan_check ok\n");
    return 0;
}
"""


def test_planner_under_asan_and_ubsan_at_the_abi_maxima(tmp_path):
    exe = _compile(tmp_path, "g16_plan_check", PLAN_CHECK, sanitize=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "groth16 plan_check ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    for src in ("zkp_groth16.hip", "zkp_pairings.hip"):
        with open(os.path.join(CSRC, src)) as f:
            assert '#include "zkp_groth16_plan.hpp"' in f.read()


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_do_not_spill():
    from test_msm_cpu import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_fr_" in n or "k_g16_" in n or "k_zero_fill" in n}
    # check_canonical, op, from_wide, fold x2 (products / plain sum), fold_finish; init, status, scalars, neg_g2, place, finish; and the fill
    # kernel that took the place of the MSM's two memsets (zkp_msm.hip)
    assert len(new) == 6 + 6 + 1, sorted(new)
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)
    assert not any("k_rlc_" in n for n in new)


def test_new_symbols_are_exported_and_refuse_a_null_context():
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.zkp_abi_version() == 4
    one = ctypes.c_int(0)
    vk, b = _lib.Groth16Vk(n_inputs=0), _lib.Groth16Batch(n=0)
    assert lib.zkp_groth16_verify_batch(None, ctypes.byref(vk), ctypes.byref(b), None, 0, ctypes.byref(one)) == -1
    assert lib.zkp_groth16_verify_batch_dev(None, ctypes.byref(vk), ctypes.byref(b), None, 0, None, None) == -1
    assert lib.zkp_fr_op_batch(None, 0, None, None, 0, None) == -1
    assert lib.zkp_fr_from_wide_batch(None, None, 0, None) == -1
    assert lib.zkp_fr_fold_batch(None, None, None, 0, 0, None, None) == -1


def test_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import synthetic
    for name in ("fr_op", "fr_from_wide", "fr_fold", "groth16_verify_batch"):
        assert callable(getattr(z.PairingEngine, name))
    assert callable(z.groth16_verify_batch) and callable(z.groth16_verify_each) and callable(synthetic.groth16_instance)
    a, b = z.Fr(R - 1), z.Fr(5)
    assert int(a + b) == 4 and int(a * b) == R - 5 and int(-b) == R - 5 and int(b - a) == 6 and int(b.invert() * b) == 1 and z.Fr(0).invert() is None
    assert int(z.Fr.from_array(z.Fr(R - 2).to_array())) == R - 2 and int(b.square()) == 25
