"""CPU gate for the KZG cell proofs (include/zkp_cells.h): the model on Python integers - the pipeline of the header against the DEFINITION
(the quotient by X^l - c^l, the cells as evaluations on cosets, the interpolant by Lagrange's formula), the degenerate cell sizes against
fk20_model, the verifier's combined equation; the planner (csrc/zkp_cells_plan.hpp) walked to the ABI maxima and its whole schedule run
over a toy group with every group size, under ASan and UBSan (tests/cells_plan_check.cpp, a child process); the group size it chooses at
the shapes of tests/cells_shapes.py; the new header, the ctypes table and the Rust file against one another; the replay table against the
header; the new kernels' registers."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import cells_model as cm
import cells_shapes
import fk20_model as fm
import poly_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "zkp_cells.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "cells.rs")
R = pm.R
TAU = 0x5EED0000000000000000000000000000000000000000000000000000C0FFEE % R
NEW = ["zkp_kzg_cells_setup", "zkp_kzg_cells_setup_dev", "zkp_kzg_cells_batch", "zkp_kzg_cells_batch_dev", "zkp_kzg_cell_verify_batch",
       "zkp_kzg_cell_verify_batch_dev"]
NAMES = r"zkp_kzg_cell"


def polys_of(n, rng):
    """dense, zero, constant, only f_{N-1}, all coefficients equal"""
    v = rng.randrange(1, R)
    return [[rng.randrange(R) for _ in range(n)], [0] * n, [v] + [0] * (n - 1), [0] * (n - 1) + [v], [v] * n]


# ------------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("log2_n", range(7))
def test_pipeline_equals_the_definition_at_every_cell_size(log2_n):
    rng = random.Random(0xCE + log2_n)
    polys = polys_of(1 << log2_n, rng)
    for log2_l in range(log2_n + 1):
        k = 1 << (log2_n - log2_l)
        for log2_ext in (0, 1):
            for bitrev in (False, True):
                for which, f in [(w, p) for w, p in enumerate(polys) if log2_n <= 4 or w in (0, 4)]:
                    got = cm.cell_proofs(f, TAU, log2_n, log2_l, log2_ext, bitrev)
                    assert got == cm.quotient_proofs(f, TAU, log2_n, log2_l, log2_ext, bitrev), (log2_n, log2_l, log2_ext, bitrev, which)
                    assert len(got) == k << log2_ext
                    if k == 1 or which in (1, 2):
                        assert not any(got)                          # l = N, the zero and the constant polynomial: every proof infinite
                if bitrev:                                           # the cells are rows of the transform of the zero-padded coefficients
                    assert cm.cell_values(polys[0], log2_n, log2_l, log2_ext, True) == cm.extended_values(polys[0], log2_n, log2_l, log2_ext, True)
        if k >= 2 and log2_n:
            assert any(cm.cell_proofs(polys[0], TAU, log2_n, log2_l, 1))


@pytest.mark.parametrize("log2_n", range(7))
def test_cells_of_one_value_are_the_fk20_single_proofs(log2_n):
    rng = random.Random(0xF1 + log2_n)
    f = [rng.randrange(R) for _ in range(1 << log2_n)]
    assert cm.cells_setup(TAU, log2_n, 0) == [fm.fk20_setup(TAU, log2_n)]
    for bitrev in (False, True):
        assert cm.cell_proofs(f, TAU, log2_n, 0, 0, bitrev) == fm.fk20_proofs(f, TAU, log2_n, bitrev)
    assert cm.c_vectors(f, 0) == [fm.c_vector(f)]
    assert cm.h_vector(f, TAU, log2_n, 0) == fm.h_vector(f, TAU, log2_n)


@pytest.mark.parametrize("log2_n,log2_l", [(4, 2), (6, 2), (3, 3), (5, 1), (1, 0)])
def test_the_vectors_of_the_pipeline_on_their_own(log2_n, log2_l):
    n, l = 1 << log2_n, 1 << log2_l
    k = n // l
    rng = random.Random(0xC1 + log2_n)
    f = [rng.randrange(1, R) for _ in range(n)]
    s = [pow(TAU, j, R) for j in range(n)]
    for i, (c, x) in enumerate(zip(cm.c_vectors(f, log2_l), cm.setup_vectors(s, log2_l))):
        assert len(c) == len(x) == 2 * k and c[0] == f[n - 1 - i] and c[1:k + 2] == [0] * min(k + 1, 2 * k - 1)
        assert c[k + 2:] == [f[d * l - 1 - i] for d in range(2, k)]
        assert x[:k - 1] == [s[n - (e + 1) * l - 1 - i] for e in range(k - 1)] and x[max(k - 1, 0):] == [0] * (k + 1)
    h = cm.h_vector(f, TAU, log2_n, log2_l)
    # h_u = sum_j f_{j + (u + 1) l} tau^j, and entry k - 1 is zero by construction (what lies behind it is the circulant's wrap-around)
    assert h[:k] == [sum(f[j + (u + 1) * l] * s[j] for j in range(n - (u + 1) * l)) % R for u in range(k)] and h[k - 1] == 0


@pytest.mark.parametrize("log2_n,log2_l,log2_ext,bitrev", [(4, 2, 1, True), (4, 2, 1, False), (3, 3, 1, True), (4, 1, 0, True), (3, 0, 1, False)])
def test_the_verifiers_equation_accepts_good_cells_and_refuses_each_corruption(log2_n, log2_l, log2_ext, bitrev):
    rng = random.Random(0x7E + log2_n + log2_l)
    big_m = 1 << (log2_n - log2_l + log2_ext)
    polys = [[rng.randrange(R) for _ in range(1 << log2_n)] for _ in range(2)]
    vals = [cm.cell_values(f, log2_n, log2_l, log2_ext, bitrev) for f in polys]
    prf = [cm.quotient_proofs(f, TAU, log2_n, log2_l, log2_ext, bitrev) for f in polys]
    com = [cm.horner(f, TAU) for f in polys]
    cells = [(com[j], m, vals[j][m], prf[j][m]) for j in range(2) for m in range(big_m)]
    rs = [rng.randrange(1, R) for _ in cells]
    shape = (TAU, log2_n, log2_l, log2_ext, bitrev)
    assert all(cm.cell_holds(c, m, v, p, *shape) for c, m, v, p in cells)              # the definition, cell by cell, Lagrange's formula
    assert cm.batch_holds(cells, rs, *shape)                                           # the combined equation, the transform's route
    for bad in (0, len(cells) // 2, len(cells) - 1):
        c, m, v, p = cells[bad]
        v2 = list(v)
        v2[-1] = (v2[-1] + 1) % R
        for what, cell in (("value", (c, m, v2, p)), ("index", (c, (m + 1) % big_m, v, p)), ("proof", (c, m, v, (p + 1) % R)), ("commitment", ((c + 1) % R, m, v, p))):
            if what == "index" and big_m == 1:
                continue
            assert not cm.cell_holds(*cell, *shape), (what, bad)
            assert not cm.batch_holds(cells[:bad] + [cell] + cells[bad + 1:], rs, *shape), (what, bad)


def test_the_exceptional_additions_need_equal_bases_and_the_gpu_tests_inputs_reach_them():
    """Equal coefficients alone give neither equal nor opposite partials - X_i[t] = tau^-i X_0[t] - whatever the group size.  Under a setup
    with tau = 1 they give the doubling in the sum and, for g > 1, inside a lane; under tau = -1 the opposite case (in the sum at g = 1,
    inside a lane for g > 1, whose partials are then infinite); sign blocks under tau = 1 give opposite partials at every g.  The shapes
    and polynomials are the ones tests/test_gpu_cells.py runs."""
    import cells_replay_cases as crc
    for n, log2_n, log2_l, log2_ext, g in cells_shapes.EXCEPTIONAL_SHAPES:
        s = g.bit_length() - 1
        polys = crc.exceptional_polys(log2_n, log2_l, s, 0xE8C + n)
        equal, blocks = polys[0], polys[1]
        ordinary = cm.addition_cases(equal, TAU, log2_n, log2_l, s)
        assert not any(ordinary[x] for x in ("mac_double", "mac_opposite", "sum_double", "sum_opposite", "sum_infinite")), ordinary
        one, minus = cm.addition_cases(equal, 1, log2_n, log2_l, s), cm.addition_cases(equal, R - 1, log2_n, log2_l, s)
        assert one["sum_double"] > 0 and one["mac_into_infinity"] > 0 and (g == 1 or one["mac_double"] > 0), (g, one)
        assert (minus["sum_opposite"] if g == 1 else minus["mac_opposite"]) > 0 and minus["sum_infinite"] > 0, (g, minus)
        assert cm.addition_cases(blocks, 1, log2_n, log2_l, s)["sum_opposite"] > 0, g
        for tau in crc.EXCEPTIONAL_TAUS:          # and the model still equals the definition under these setups
            for f in polys[:3]:
                assert cm.cell_proofs(f, tau, log2_n, log2_l, log2_ext, True) == cm.quotient_proofs(f, tau, log2_n, log2_l, log2_ext, True)
    assert [sh[4] for sh in cells_shapes.EXCEPTIONAL_SHAPES] == list(cells_shapes.G_VALUES)


# ------------------------------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cells_plan") / "cells_plan_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         "-o", exe, os.path.join(ROOT, "tests", "cells_plan_check.cpp")], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _clean(out):
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]


def test_planner_holds_at_the_abi_maxima_and_its_schedule_computes_the_proofs(plan_exe):
    out = subprocess.run([plan_exe], capture_output=True, text=True, timeout=900)
    _clean(out)
    assert re.search(r"cells plan_check ok: \d+ cases", out.stdout)
    for src, inc in (("zkp_cells.hip", "zkp_cells.hpp"), ("zkp_pairings.hip", "zkp_cells.hpp"), ("zkp_cells.hpp", "zkp_cells_plan.hpp"), ("zkp_coop.hpp", "zkp_cells_plan.hpp")):
        with open(os.path.join(CSRC, src)) as f:
            assert '#include "%s"' % inc in f.read(), src
    with open(os.path.join(CSRC, "zkp_cells_plan.hpp")) as f:
        text = f.read()
    assert "hip_runtime" not in text and "getenv" not in text                          # host-only text, and no knob selects g


def test_the_shapes_of_cells_shapes_reach_every_group_size(plan_exe):
    """the planner's own answer for the shapes test_gpu_cells.py runs: what the table says, and every value g can take"""
    lines = "".join("%d %d %d\n" % s[:3] for s in cells_shapes.G_SHAPES)
    out = subprocess.run([plan_exe, "shapes"], input=lines, capture_output=True, text=True, timeout=900)
    _clean(out)
    rows = [tuple(int(x) for x in line.split())[:4] for line in out.stdout.split("\n") if line]
    assert rows == [s[:3] + (s[4],) for s in cells_shapes.G_SHAPES], out.stdout
    assert {r[3] for r in rows} == set(cells_shapes.G_VALUES)
    with open(os.path.join(CSRC, "zkp_cells_plan.hpp")) as f:
        assert int(re.search(r"G_MAX_LOG2 = (\d+);", f.read()).group(1)) == max(cells_shapes.G_VALUES).bit_length() - 1
    assert any(s[4] == 1 << s[2] for s in cells_shapes.G_SHAPES) and any(1 < s[4] < 1 << s[2] for s in cells_shapes.G_SHAPES)     # with and without partials


def test_the_sliced_call_of_the_gpu_test_crosses_a_slice_boundary(plan_exe):
    """the slice length the GPU test assumes is the planner's for its exact shape, two slices with a short last one; rows behind the boundary
    differ from the rows at offset 0, and the expected bytes read with a wrong offset differ in both output arrays (tests/slice_pools.py)"""
    import cells_replay_cases as crc
    import slice_pools as sp
    out = subprocess.run([plan_exe, "shapes"], input="%d %d %d\n" % (crc.SLICE_N, crc.SLICE_LOG2, crc.SLICE_LOG2_L), capture_output=True, text=True, timeout=900)
    _clean(out)
    assert int(out.stdout.split()[4]) == crc.SLICE_LEN == (1 << 17) >> crc.SLICE_LOG2
    with open(HEADER) as f:
        assert "floor(2^17 / N)" in f.read()
    call = crc.slice_call(True)
    assert call.starts == [0, crc.SLICE_LEN] and call.tail == 3 and set(call.idx[-3:]) == set(crc.SLICE_TAIL) and not set(call.idx[:-3]) & set(crc.SLICE_TAIL)
    w = sp.window(call, call.starts[1])
    for name, (arr, per) in list(call.inputs.items()) + list(call.outputs.items()):
        assert sp.rows(arr, per, call.starts[1], w).tobytes() != sp.rows(arr, per, 0, w).tobytes(), name
    for name in call.outputs:
        for how in ("zero", "previous"):
            assert sp.reading(call, name, how).tobytes() != call.want(name).tobytes(), (name, how)
    assert call.pool["inf"].any() and not call.pool["inf"].all()                       # identity proofs and finite ones in the pool


# ------------------------------------------------------------------------------------------------------------------- the boundary
def _header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _declared_symbols():
    return sorted(set(re.findall(r"\b(zkp_[a-z0-9_]+)\s*\(", _header_text())))


def _split_params(txt):
    txt = txt.strip()
    return [] if txt in ("", "void") else [p.strip() for p in txt.split(",")]


def _c_signatures():
    def kind(t):
        if "*" in t:
            return "ptr"
        if "size_t" in t:
            return "size"
        if re.search(r"\b(int|unsigned|uint32_t)\b", t):
            return "int"
        assert t.strip() == "void", t
        return "void"
    return {name: (kind(ret), [kind(p) for p in _split_params(params)])
            for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(zkp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_text())}


def _rust_signatures():
    def kind(t):
        t = t.strip()
        if t.startswith("*"):
            return "ptr"
        if t == "usize":
            return "size"
        assert t in ("c_int", "c_uint", "u32", "i32"), t
        return "int"
    with open(RUST) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    out = {}
    for name, params, ret in re.findall(r"pub fn (zkp_[a-z0-9_]+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", text):
        out[name] = ("void" if not ret.strip() else kind(ret), [kind(p.split(":", 1)[1]) for p in _split_params(params)])
    return out


def test_header_ctypes_and_rust_agree_and_every_symbol_is_exported():
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    names = _declared_symbols()
    assert names == sorted(NEW)
    c = _c_signatures()
    assert sorted(c) == names and sorted(_lib.CELLS_SIGNATURES) == names
    rust = _rust_signatures()
    assert sorted(rust) == names
    for name, sig in c.items():
        assert hasattr(lib, name), "libzkp_pairings.so does not export %s" % name
        assert rust[name] == sig, (name, "rust", rust[name], "header", sig)
        if name.endswith("_dev"):
            assert sig[1][-1] == "ptr" and c[name[:-4]] == (sig[0], sig[1][:-1]), name          # the host flavour plus a trailing stream

    def ckind(t):
        if t is None:
            return "void"
        if t is ctypes.c_size_t:
            return "size"
        if t in (ctypes.c_int, ctypes.c_uint, ctypes.c_uint32):
            return "int"
        assert t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer), t
        return "ptr"
    for name, (res, args) in _lib.CELLS_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args                                   # load() bound the fifth table as well
    tables = [_lib.SIGNATURES, _lib.POLY_SIGNATURES, _lib.PROVE_SIGNATURES, _lib.FK20_SIGNATURES, _lib.CELLS_SIGNATURES]
    assert sum(len(t) for t in tables) == len(set().union(*tables))                  # the five tables are disjoint
    assert lib.zkp_abi_version() == 4
    with open(HEADER) as f:
        h = f.read()
    assert (int(re.search(r"#define ZKP_CELLS_POINTS_CHECKED (\d+)", h).group(1)), int(re.search(r"#define ZKP_CELLS_VK_CHECKED (\d+)", h).group(1))) == \
        (_lib.CELLS_POINTS_CHECKED, _lib.CELLS_VK_CHECKED)
    assert not (_lib.CELLS_POINTS_CHECKED | _lib.CELLS_VK_CHECKED) & _lib.NTT_BITREV     # the verifier takes ZKP_NTT_BITREV beside them


def test_the_old_boundary_gained_one_comment_and_one_module_line():
    with open(os.path.join(ROOT, "include", "zkp_pairings.h")) as f:
        old = f.read()
    assert old.count("zkp_cells.h") == 1 and not any(n + "(" in old for n in NEW) and not re.search(NAMES, old)
    for other in ("zkp_poly.h", "zkp_prove.h", "zkp_fk20.h"):
        with open(os.path.join(ROOT, "include", other)) as f:
            assert not re.search(NAMES + "|zkp_cells", f.read()), other
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert len(re.findall(r"^(?:pub )?mod cells;$", lib_rs, re.M)) == 1 and not re.search(NAMES, lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_cells.hip", "zkp_cells.hpp", "zkp_cells_plan.hpp", "include/zkp_cells.h"))
    assert os.path.exists(os.path.join(ROOT, "integration", "c", "zkp_cells.c"))
    with open(HEADER) as f:
        h = f.read()
    assert all(x in h for x in ("zkp_g1_is_valid_batch", "TRUSTED", "under ABI version 4", "Slices and workspace", "Cost:", "How", "ZKP_ERR_ARG"))


def test_every_dev_entry_point_of_the_new_header_has_a_replay_case_or_a_written_reason():
    import cells_replay_cases as crc
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(zkp_\w+_dev)\(", f.read()))
    table, excluded = crc.table_c_names(), set(crc.EXCLUDED)
    assert declared == {n for n in NEW if n.endswith("_dev")}
    assert not (table & excluded)
    assert declared - (table | excluded) == set(), "no replay case and no reason: %s" % sorted(declared - (table | excluded))
    assert (table | excluded) - declared == set(), "not declared in the header: %s" % sorted((table | excluded) - declared)
    assert all(isinstance(why, str) and len(why) > 20 for why in crc.EXCLUDED.values())
    ids = [c.id for c in crc.CASES]
    assert len(ids) == len(set(ids))
    from zkvm_pairings_amd.engine import PairingEngine
    for c in crc.CASES:
        assert c.c_names and callable(getattr(PairingEngine, c.method)) and len(c.shape) == len(c.small), c.id
    assert {c.method for c in crc.CASES} == {"kzg_cells_setup", "kzg_cells", "kzg_cell_verify"}


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_are_there_and_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_cell_" in n}
    # mac, sum; coeffs; the verifier's scale and place (its flag and G2-side launches are the KZG verifier's)
    assert len(new) == 5, sorted(new)
    for part in ("k_cell_mac", "k_cell_sum", "k_cell_coeffs", "k_cell_scale", "k_cell_place"):
        assert sum(part in n for n in new) == 1, part
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgpr"] <= 256, (n, v)
    mac = [v for n, v in new.items() if "k_cell_mac" in n][0]
    assert mac["lds"] == 0, mac                                                        # dynamic: g x 8 KiB per launch (cells::mac_lds_bytes)
    with open(os.path.join(CSRC, "zkp_cells_plan.hpp")) as f:
        assert "mac_lds_bytes(uint32_t s) { return (2u << s) * 4 * 64 * 16; }" in f.read()
    # no name of the new kernels contains what an older gate counts by
    counted = ("k_ntt_pass", "k_msm_", "k_add28", "k_g1_mul_endo28", "k_fr_", "k_kzg_", "k_prove_", "k_spmv", "k_poly_coset", "k_open_quot", "k_rlc_",
               "k_g16_", "k_frinv_", "k_freval_", "k_zero_fill", "k_coop", "k_g1ntt_", "k_fk20_")
    assert not [n for n in new for x in counted if x in n]
    # the transforms the cell calls drive kept their registers and LDS: the figures of the commit before this header
    want = {"k_g1ntt_stage": (239, 24576), "k_g1ntt_scale": (224, 24576), "k_g1ntt_out": (128, 0), "k_fk20_mul": (208, 8192), "k_g1ntt_firstILi2": (210, 12288),
            "k_g1ntt_firstILi0": (209, 12288), "k_g1_mul28": (208, 8192)}
    for part, (vgpr, lds) in want.items():
        hit = [v for n, v in k.items() if part in n]
        assert len(hit) == 1 and (hit[0]["vgpr"], hit[0]["lds"], hit[0]["spill"], hit[0]["scratch"]) == (vgpr, lds, 0, 0), (part, hit)


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    assert lib.zkp_kzg_cells_setup(None, None, 0, 0, None, None) == -1 and lib.zkp_kzg_cells_setup_dev(None, None, 0, 0, None, None, None) == -1
    assert lib.zkp_kzg_cells_batch(None, None, None, None, 0, 0, 0, 0, 0, None, None) == -1
    assert lib.zkp_kzg_cells_batch_dev(None, None, None, None, 0, 0, 0, 0, 0, None, None, None) == -1
    ok = ctypes.c_int(0)
    okp = ctypes.cast(ctypes.byref(ok), ctypes.c_void_p)
    assert lib.zkp_kzg_cell_verify_batch(None, *([None] * 9), 0, 0, 0, 0, None, okp) == -1
    assert lib.zkp_kzg_cell_verify_batch_dev(None, *([None] * 9), 0, 0, 0, 0, None, okp, None) == -1
    for name in ("kzg_cells_setup", "kzg_cells", "kzg_cell_verify"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("CellSetup", "kzg_cells_setup", "kzg_cell_proofs_batch", "kzg_cells_and_proofs_batch", "kzg_cell_verify_batch", "kzg_cell_verify_each"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.synthetic.kzg_cells_instance)
