"""CPU gate for the G1 NTT and FK20 (include/zkp_fk20.h): the model on Python integers - the circulant pipeline against the quotient
formula, the vector c, the setup vector, "entry N - 1 of h is zero", the inverse transform of tau^k against l_i(tau); the twiddle split
through the table-building kernel's own arithmetic on the host; the planner (csrc/zkp_fk20_plan.hpp) walked to the ABI maxima and its
whole schedule run over a toy group under ASan and UBSan (tests/fk20_plan_check.cpp, a child process); the new header, the ctypes table
and the Rust file against one another; the replay table against the header; the new kernels' registers."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import fk20_model as fm
import poly_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "zkp_fk20.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "fk20.rs")
R = pm.R
TAU = 0x5EED0000000000000000000000000000000000000000000000000000C0FFEE % R
NEW = ["zkp_g1_ntt_batch", "zkp_g1_ntt_batch_dev", "zkp_kzg_fk20_setup", "zkp_kzg_fk20_setup_dev", "zkp_kzg_fk20_batch", "zkp_kzg_fk20_batch_dev"]
NAMES = r"zkp_(g1_ntt|kzg_fk20)"


# ------------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("log2_n", [0, 1, 2, 3, 6])
def test_circulant_pipeline_equals_the_quotient_formula(log2_n):
    n = 1 << log2_n
    rng = random.Random(0xF0 + log2_n)
    polys = [[rng.randrange(R) for _ in range(n)], [0] * n, [rng.randrange(1, R)] + [0] * (n - 1), [0] * (n - 1) + [rng.randrange(1, R)],
             [rng.randrange(1, R)] + [0] * (n - 2) + [rng.randrange(1, R)] if n > 1 else [5]]
    for which, f in enumerate(polys):
        for bitrev in (False, True):
            assert fm.fk20_proofs(f, TAU, log2_n, bitrev) == fm.quotient_proofs(f, TAU, log2_n, bitrev), (log2_n, which, bitrev)
        if which in (1, 2):
            assert not any(fm.fk20_proofs(f, TAU, log2_n))                       # the zero and the constant polynomials: every proof infinite
    if n > 1:
        assert any(fm.fk20_proofs(polys[0], TAU, log2_n))


@pytest.mark.parametrize("log2_n", [0, 1, 2, 3, 6])
def test_the_vectors_of_the_pipeline_on_their_own(log2_n):
    n = 1 << log2_n
    rng = random.Random(0xC0 + log2_n)
    f = [rng.randrange(1, R) for _ in range(n)]
    c = fm.c_vector(f)
    assert len(c) == 2 * n and c[0] == f[n - 1] and c[1:n + 2] == [0] * min(n + 1, 2 * n - 1) and c[n + 2:] == f[1:n - 1]
    s = [pow(TAU, k, R) for k in range(n)]
    x = fm.setup_vector(s)
    assert len(x) == 2 * n and x[:n - 1] == s[:n - 1][::-1] and x[max(n - 1, 0):] == [0] * (n + 1)
    u = fm.h_vector(f, TAU, log2_n)
    # h_i = sum_{m > i} f_m tau^(m - i - 1), and entry N - 1 is zero by construction
    assert u[:n] == [sum(f[m] * s[m - i - 1] for m in range(i + 1, n)) % R for i in range(n)] and u[n - 1] == 0
    # the same pipeline from the definition of the transform, not the fast one
    if log2_n <= 3:
        assert pm.ntt_definition(fm.setup_vector(s), log2_n + 1) == fm.fk20_setup(TAU, log2_n)


@pytest.mark.parametrize("log2_n", [0, 1, 2, 3, 6])
def test_inverse_transform_of_the_monomial_setup_is_the_lagrange_setup(log2_n):
    n = 1 << log2_n
    s = [pow(TAU, k, R) for k in range(n)]
    lag = fm.lagrange_at(TAU, log2_n)
    assert pm.ntt(s, log2_n, inverse=True) == lag and sum(lag) % R == 1
    for bitrev in (False, True):
        # [l_i(tau)] for the point of slot i: what kzg_commit_batch pairs with evaluations in that order
        f = [random.Random(log2_n).randrange(R) for _ in range(n)]
        ev = pm.ntt(f, log2_n, bitrev=bitrev)
        slot = [lag[pm.bit_reverse(i, log2_n)] if bitrev else lag[i] for i in range(n)]
        assert sum(a * b for a, b in zip(ev, slot)) % R == fm.horner(f, TAU)


# ------------------------------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fk20_plan") / "fk20_plan_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         "-o", exe, os.path.join(ROOT, "tests", "fk20_plan_check.cpp")], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _clean(out):
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]


def test_planner_holds_at_the_abi_maxima_and_its_schedule_computes_the_transform(plan_exe):
    out = subprocess.run([plan_exe], capture_output=True, text=True, timeout=900)
    _clean(out)
    assert re.search(r"fk20 plan_check ok: \d+ cases", out.stdout)
    for src in ("zkp_fk20.hip", "zkp_pairings.hip", "zkp_coop.hpp"):
        with open(os.path.join(CSRC, src)) as f:
            assert "zkp_fk20_plan.hpp" in f.read(), src
    with open(os.path.join(CSRC, "zkp_fk20_plan.hpp")) as f:
        assert "hip_runtime" not in f.read()                                      # host-only text


def test_twiddle_split_of_every_domain_up_to_2_11(plan_exe):
    """a + b z^2 == w^t (mod r) and a, b < 2^128 for every entry of the 2^11-point domain (the smaller domains are its strides), and for
    the scalings 2^-k: split_z2 itself, the function k_g1ntt_split calls, replayed on the host"""
    dom = pm.domain(11)
    for k in range(12):
        assert pm.domain(k) == dom[::1 << (11 - k)]
    vals = dom + [pow(1 << k, -1, R) for k in range(21)] + [0, 1, R - 1, fm.Z2 - 1, fm.Z2, fm.Z2 + 1]
    out = subprocess.run([plan_exe, "split"], input="".join("%064x\n" % v for v in vals), capture_output=True, text=True, timeout=900)
    _clean(out)
    rows = [tuple(int(x, 16) for x in line.split()) for line in out.stdout.split("\n") if line]
    assert len(rows) == len(vals)
    for v, (a, b) in zip(vals, rows):
        assert (a + b * fm.Z2) % R == v and a < 1 << 128 and b < 1 << 128 and (a, b) == fm.split(v), hex(v)
    assert max(b for _, b in rows) > 1 << 126                                      # the high half is really used


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
    assert sorted(c) == names and sorted(_lib.FK20_SIGNATURES) == names
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
    for name, (res, args) in _lib.FK20_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args                                   # load() bound the fourth table as well
    tables = [_lib.SIGNATURES, _lib.POLY_SIGNATURES, _lib.PROVE_SIGNATURES, _lib.FK20_SIGNATURES]
    assert sum(len(t) for t in tables) == len(set().union(*tables))                  # the four tables are disjoint
    assert lib.zkp_abi_version() == 4


def test_the_old_boundary_gained_one_comment_and_one_module_line():
    with open(os.path.join(ROOT, "include", "zkp_pairings.h")) as f:
        old = f.read()
    assert old.count("zkp_fk20.h") == 1 and not any(n + "(" in old for n in NEW) and not re.search(NAMES, old)
    for other in ("zkp_poly.h", "zkp_prove.h"):
        with open(os.path.join(ROOT, "include", other)) as f:
            assert not re.search(NAMES + "|zkp_fk20", f.read()), other
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert len(re.findall(r"^(?:pub )?mod fk20;$", lib_rs, re.M)) == 1 and not re.search(NAMES, lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_fk20.hip", "zkp_fk20.hpp", "zkp_fk20_plan.hpp", "include/zkp_fk20.h"))
    assert os.path.exists(os.path.join(ROOT, "integration", "c", "zkp_fk20.c"))
    with open(HEADER) as f:
        h = f.read()
    assert all(x in h for x in ("zkp_g1_is_valid_batch", "TRUSTED", "under ABI version 4", "Slices and workspace", "Cost:", "How"))


def test_every_dev_entry_point_of_the_new_header_has_a_replay_case_or_a_written_reason():
    import fk20_replay_cases as frc
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(zkp_\w+_dev)\(", f.read()))
    table, excluded = frc.table_c_names(), set(frc.EXCLUDED)
    assert declared == {n for n in NEW if n.endswith("_dev")}
    assert not (table & excluded)
    assert declared - (table | excluded) == set(), "no replay case and no reason: %s" % sorted(declared - (table | excluded))
    assert (table | excluded) - declared == set(), "not declared in the header: %s" % sorted((table | excluded) - declared)
    assert all(isinstance(why, str) and len(why) > 20 for why in frc.EXCLUDED.values())
    ids = [c.id for c in frc.CASES]
    assert len(ids) == len(set(ids))
    from zkvm_pairings_amd.engine import PairingEngine
    for c in frc.CASES:
        assert c.c_names and callable(getattr(PairingEngine, c.method)) and len(c.shape) == len(c.small), c.id
    # N = 64 with three vectors or polynomials, a smaller eager call at N = 4 with one
    assert {c.method: (c.shape[:2], c.small[:2]) for c in frc.CASES} == {"g1_ntt": ((3, 6), (1, 2)), "kzg_fk20_setup": ((6,), (2,)), "kzg_fk20": ((3, 6), (1, 2))}


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_are_there_and_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_g1ntt_" in n or "k_fk20_" in n}
    # first (from the wire, from records), stage, scale, out, split; coeffs, mul
    assert len(new) == 8 and sum("k_g1ntt_first" in n for n in new) == 2, sorted(new)
    for part in ("k_g1ntt_stage", "k_g1ntt_scale", "k_g1ntt_out", "k_g1ntt_split", "k_fk20_coeffs", "k_fk20_mul"):
        assert sum(part in n for n in new) == 1, part
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgpr"] <= 256, (n, v)       # two waves per SIMD at the most
    stage = [v for n, v in new.items() if "k_g1ntt_stage" in n][0]
    assert stage["lds"] == 6 * 4 * 64 * 16, stage                                    # B and B + phi'(B): six values of four quads per lane
    # no name of the new kernels contains what an older gate counts by
    counted = ("k_ntt_pass", "k_msm_", "k_add28", "k_g1_mul_endo28", "k_fr_", "k_kzg_", "k_prove_", "k_spmv", "k_poly_coset", "k_open_quot", "k_rlc_",
               "k_g16_", "k_frinv_", "k_freval_", "k_zero_fill", "k_coop")
    assert not [n for n in new for x in counted if x in n]
    # the kernels the older gates name kept their registers and LDS: the figures of the commit before this header
    want = {"k_g1_mul_endo28": (224, 20480), "k_g1_mul28": (208, 8192), "k_add28ILi1": (202, 8192), "k_msm_reduceILi1": (244, 24576),
            "k_ntt_passILb0": (155, 32768), "k_open_quot": (88, 9216)}
    for part, (vgpr, lds) in want.items():
        hit = [v for n, v in k.items() if part in n]
        assert len(hit) == 1 and (hit[0]["vgpr"], hit[0]["lds"], hit[0]["spill"], hit[0]["scratch"]) == (vgpr, lds, 0, 0), (part, hit)


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    assert lib.zkp_g1_ntt_batch(None, None, None, 0, 0, 0, None, None) == -1 and lib.zkp_g1_ntt_batch_dev(None, None, None, 0, 0, 0, None, None, None) == -1
    assert lib.zkp_kzg_fk20_setup(None, None, 0, None, None) == -1 and lib.zkp_kzg_fk20_setup_dev(None, None, 0, None, None, None) == -1
    assert lib.zkp_kzg_fk20_batch(None, None, None, None, 0, 0, 0, None, None) == -1
    assert lib.zkp_kzg_fk20_batch_dev(None, None, None, None, 0, 0, 0, None, None, None) == -1
    for name in ("g1_ntt", "kzg_fk20_setup", "kzg_fk20"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("g1_ntt", "Fk20Setup", "kzg_fk20_setup", "kzg_open_domain_batch", "kzg_lagrange_setup"):
        assert callable(getattr(z, name)) and name in z.__all__
