"""CPU gate for the polynomial / producer layer (include/zkp_poly.h): the Python model of the NTT against its definition; the schedule
of the device transform replayed on the host (tests/poly_plan_check.cpp: every pass run from csrc/zkp_poly_plan.hpp's index functions,
built with ASan and UBSan, run as a child process) against that model, byte for byte; the kernels' own text on host threads
(tests/poly_kernel_host.cpp); the quotient formulas of the opening; the new header, the ctypes table and the Rust
file against one another; the replay table against the header; the new kernels' registers."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import poly_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "zkp_poly.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "poly.rs")
R = pm.R
NEW = ["zkp_fr_ntt_batch", "zkp_fr_ntt_batch_dev", "zkp_kzg_open_batch", "zkp_kzg_open_batch_dev"]


# ------------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("log2_n", range(7))
def test_model_against_the_definition(log2_n):
    rng = random.Random(0x0DE + log2_n)
    n = 1 << log2_n
    for vals in ([rng.randrange(R) for _ in range(n)], [R - 1] * n, [0] * (n - 1) + [1]):
        for bitrev in (False, True):
            for coset in (False, True):
                fwd = pm.ntt(vals, log2_n, bitrev=bitrev, coset=coset)
                assert fwd == pm.ntt_definition(vals, log2_n, bitrev=bitrev, coset=coset), (log2_n, bitrev, coset)
                assert pm.ntt(fwd, log2_n, inverse=True, bitrev=bitrev, coset=coset) == vals
                assert pm.ntt(pm.ntt(vals, log2_n, inverse=True, bitrev=bitrev, coset=coset), log2_n, bitrev=bitrev, coset=coset) == vals
    from zkvm_pairings_amd import synthetic
    assert pm.root_of_unity(log2_n) == synthetic.fr_root_of_unity(log2_n)
    assert [pm.bit_reverse(i, log2_n) for i in range(n)] == [synthetic.bit_reverse(i, log2_n) for i in range(n)]


def test_model_round_trip_at_a_two_pass_size():
    rng = random.Random(0x0DF)
    vals = [rng.randrange(R) for _ in range(1 << 11)]
    for flags in (0, pm.BITREV, pm.COSET, pm.BITREV | pm.COSET):
        assert pm.ntt_flags(pm.ntt_flags(vals, 11, flags), 11, flags | pm.INVERSE) == vals


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("log2_n", [0, 1, 3, 4])
def test_quotient_formulas_of_the_opening_against_tau(log2_n, bitrev):
    """what k_open_quot computes, on Python integers: q_i = (y - f_i) / (z - w^idx(i)) outside the domain; for z = w^idx(m), q_m =
    -w^(N - idx(m)) sum_i q_i w^idx(i) with q_m = 0 inside the sum.  sum_i q_i l_i(tau) must be (f(tau) - y) / (tau - z): the proof's
    exponent against a Lagrange setup in the order of the evaluations."""
    rng = random.Random(0x90 + log2_n)
    n = 1 << log2_n
    dom = pm.domain(log2_n)
    idx = [pm.bit_reverse(i, log2_n) if bitrev else i for i in range(n)]
    tau = rng.randrange(R)
    lag = [(pow(tau, n, R) - 1) * pow(n, -1, R) * dom[idx[i]] * pow(tau - dom[idx[i]], -1, R) % R for i in range(n)]
    horner = lambda c, x: sum(v * pow(x, k, R) for k, v in enumerate(c)) % R
    for coeffs in ([rng.randrange(R) for _ in range(n)], [0] * n, [5] + [0] * (n - 1), [0] * (n - 1) + [3]):
        f = pm.ntt(coeffs, log2_n, bitrev=bitrev)
        for z, m in [(rng.randrange(R), None), (0, None)] + [(dom[idx[m]], m) for m in range(n)]:
            y = horner(coeffs, z)
            assert m is None or y == f[m]
            q = [0 if i == m else (y - f[i]) * pow(z - dom[idx[i]], -1, R) % R for i in range(n)]
            if m is not None:
                q[m] = -dom[(n - idx[m]) % n] * sum(q[i] * dom[idx[i]] for i in range(n)) % R
            assert sum(a * b for a, b in zip(q, lag)) % R == (horner(coeffs, tau) - y) * pow(tau - z, -1, R) % R, (log2_n, bitrev, m)


# ------------------------------------------------------------------------------------------------------------------- the schedule
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("poly_plan") / "poly_plan_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         "-o", exe, os.path.join(ROOT, "tests", "poly_plan_check.cpp")], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


# the tile of the product (2^10) over every size from 0 to 14; smaller tiles run the same functions through plans of up to seven
# passes, three-pass plans with and without the top pass among them
@pytest.mark.parametrize("t,kmax", [(10, 14), (4, 9), (5, 10), (7, 12)])
def test_host_replay_of_the_schedule_equals_the_model(plan_exe, tmp_path, t, kmax):
    rng = random.Random(0x5C4ED + t)
    vals = [rng.randrange(R) for _ in range(3 << kmax)]
    vals[0], vals[1], vals[2] = R - 1, 0, 1
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(pm.to_bytes(vals))
    out = subprocess.run([plan_exe, str(fin), str(fout), str(t), str(kmax)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "poly plan_check ok: %d cases" % (16 * (kmax + 1)) in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    got = fout.read_bytes()
    at = 0
    for k in range(kmax + 1):
        n = 1 << k
        for flags in range(8):
            want = [pm.to_bytes(pm.ntt_flags(vals[j * n:(j + 1) * n], k, flags)) for j in range(3)]
            for n_poly in (1, 3):
                w = b"".join(want[:n_poly])
                assert got[at:at + len(w)] == w, (t, k, flags, n_poly)
                at += len(w)
    assert at == len(got)
    for src in ("zkp_poly.hip", "zkp_pairings.hip"):
        with open(os.path.join(CSRC, src)) as f:
            assert '#include "zkp_poly_plan.hpp"' in f.read()


# ------------------------------------------------------------------------------------------------------------------- the kernels' own text
@pytest.fixture(scope="module")
def kernel_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("poly_kernels") / "poly_kernel_host")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                         "-Wno-unknown-pragmas", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "poly_kernel_host.cpp")], capture_output=True, text=True,
                        timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _kernel_run(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]


@pytest.mark.parametrize("log2_n,n_poly", [(0, 3), (1, 5), (3, 3), (9, 3), (10, 1), (11, 1), (12, 2)])
def test_ntt_kernels_on_host_threads_equal_the_model(kernel_exe, tmp_path, log2_n, n_poly):
    """k_ntt_pass and k_poly_coset as written in zkp_poly.hip, one host thread per lane: below a wavefront, a partial tile, t - 1, t,
    t + 1, the 4096-point size; every flag combination, out of place and in place"""
    rng = random.Random(0xE30 + log2_n)
    n = 1 << log2_n
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(n_poly)]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(pm.to_bytes([v for p in polys for v in p]))
    for flags in range(8):
        want = pm.to_bytes([v for p in polys for v in pm.ntt_flags(p, log2_n, flags)])
        for inplace in ([], ["inplace"]):
            _kernel_run(kernel_exe, ["ntt", fin, fout, log2_n, n_poly, flags] + inplace)
            assert fout.read_bytes() == want, (log2_n, n_poly, flags, inplace)


@pytest.mark.parametrize("bitrev", [0, 1])
@pytest.mark.parametrize("log2_n,n", [(0, 3), (1, 2), (3, 5), (8, 3), (9, 2), (12, 1)])
def test_quotient_kernel_on_host_threads(kernel_exe, tmp_path, log2_n, n, bitrev):
    """k_open_quot as written: every second polynomial is opened inside the domain, at a random slot"""
    rng = random.Random(0xE31 + log2_n + bitrev)
    big_n = 1 << log2_n
    dom = pm.domain(log2_n)
    idx = [pm.bit_reverse(i, log2_n) if bitrev else i for i in range(big_n)]
    fs, ys, ds, want = [], [], [], []
    for j in range(n):
        c = [rng.randrange(R) for _ in range(big_n)]
        f = pm.ntt(c, log2_n, bitrev=bool(bitrev))
        m = None if j % 2 == 0 else rng.randrange(big_n)
        z = rng.randrange(R) if m is None else dom[idx[m]]
        y = 0
        for v in reversed(c):
            y = (y * z + v) % R
        dinv = [0 if i == m else pow(z - dom[idx[i]], -1, R) for i in range(big_n)]
        q = [(y - f[i]) * dinv[i] % R for i in range(big_n)]
        if m is not None:
            q[m] = -dom[(big_n - idx[m]) % big_n] * sum(q[i] * dom[idx[i]] for i in range(big_n)) % R
        fs += f
        ys.append(y)
        ds += dinv
        want += q
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(pm.to_bytes(fs) + pm.to_bytes(ys) + pm.to_bytes(ds))
    _kernel_run(kernel_exe, ["quot", fin, fout, log2_n, n, bitrev])
    assert fout.read_bytes() == pm.to_bytes(want), (log2_n, n, bitrev)


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
    with open(RUST) as f:
        text = re.sub(r"//[^\n]*", "", f.read())

    def kind(t):
        t = t.strip()
        if t.startswith("*"):
            return "ptr"
        if t == "usize":
            return "size"
        assert t in ("c_int", "c_uint", "u32", "i32"), t
        return "int"
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
    assert sorted(c) == names and sorted(_lib.POLY_SIGNATURES) == names
    rust = _rust_signatures()
    assert sorted(rust) == names
    for name, sig in c.items():
        assert hasattr(lib, name), "libzkp_pairings.so does not export %s" % name
        assert rust[name] == sig, (name, "rust", rust[name], "header", sig)

    def ckind(t):
        if t is None:
            return "void"
        if t is ctypes.c_size_t:
            return "size"
        if t in (ctypes.c_int, ctypes.c_uint, ctypes.c_uint32):
            return "int"
        assert t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer), t
        return "ptr"
    for name, (res, args) in _lib.POLY_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args                                   # load() bound the second table as well
    assert not set(_lib.POLY_SIGNATURES) & set(_lib.SIGNATURES)
    assert lib.zkp_abi_version() == 4
    # the flags: header, ctypes, Rust
    with open(HEADER) as f:
        h = f.read()
    with open(RUST) as f:
        r = f.read()
    for name, v in (("ZKP_NTT_INVERSE", _lib.NTT_INVERSE), ("ZKP_NTT_BITREV", _lib.NTT_BITREV), ("ZKP_NTT_COSET", _lib.NTT_COSET)):
        assert re.search(r"#define %s\s+%d\b" % (name, v), h) and re.search(r"pub const %s: c_int = %d;" % (name, v), r), name
    assert (_lib.NTT_INVERSE, _lib.NTT_BITREV, _lib.NTT_COSET) == (pm.INVERSE, pm.BITREV, pm.COSET) == (1, 2, 4)


def test_the_old_boundary_gained_one_comment_and_one_module_line():
    """include/zkp_pairings.h points at the new header without naming a call (the replay gate reads comments too); lib.rs declares the
    module and no new entry point"""
    with open(os.path.join(ROOT, "include", "zkp_pairings.h")) as f:
        old = f.read()
    assert "zkp_poly.h" in old and not any(n + "(" in old for n in NEW) and not re.search(r"zkp_(fr_ntt|kzg_open)", old)
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert re.search(r"^(pub )?mod poly;$", lib_rs, re.M) and not re.search(r"zkp_(fr_ntt|kzg_open)", lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_poly.hip", "zkp_poly.hpp", "zkp_poly_plan.hpp", "include/zkp_poly.h"))
    with open(HEADER) as f:
        h = f.read()
    assert "zkp_g1_is_valid_batch" in h and "zkp_g1_msm_batch" in h and "shared_bases = 1" in h and "under ABI version 4" in h


def test_every_dev_entry_point_of_the_new_header_has_a_replay_case_or_a_written_reason():
    import poly_replay_cases as prc
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(zkp_\w+_dev)\(", f.read()))
    table, excluded = prc.table_c_names(), set(prc.EXCLUDED)
    assert declared == {n for n in NEW if n.endswith("_dev")}
    assert not (table & excluded)
    assert declared - (table | excluded) == set(), "no replay case and no reason: %s" % sorted(declared - (table | excluded))
    assert (table | excluded) - declared == set(), "not declared in the header: %s" % sorted((table | excluded) - declared)
    assert all(isinstance(why, str) and len(why) > 20 for why in prc.EXCLUDED.values())
    ids = [c.id for c in prc.CASES]
    assert len(ids) == len(set(ids))
    from zkvm_pairings_amd.engine import PairingEngine
    for c in prc.CASES:
        assert c.c_names and callable(getattr(PairingEngine, c.method)) and len(c.shape) == len(c.small), c.id
    shapes = {c.method: (c.shape[:2], c.small[:2]) for c in prc.CASES}
    assert shapes == {"fr_ntt": ((5, 12), (2, 4)), "kzg_open": ((3, 8), (1, 2))}          # N = 256 and N = 4 as log2


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_ntt_pass" in n or "k_poly_coset" in n or "k_open_quot" in n}
    assert len(new) == 2 + 1 + 1, sorted(new)                  # the pass in both decimations, the coset tables, the quotient
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)
    for n, v in new.items():
        if "k_ntt_pass" in n:
            assert v["vgpr"] <= 168 and v["lds"] == 8 * 1024 * 4, (n, v)         # three waves per SIMD; the tile


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    assert lib.zkp_fr_ntt_batch(None, None, 0, 0, 0, None) == -1 and lib.zkp_fr_ntt_batch_dev(None, None, 0, 0, 0, None, None) == -1
    assert lib.zkp_kzg_open_batch(None, None, None, None, 0, 0, 0, None, None, None) == -1
    assert lib.zkp_kzg_open_batch_dev(None, None, None, None, 0, 0, 0, None, None, None, None) == -1
    for name in ("fr_ntt", "kzg_open"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("kzg_commit_batch", "kzg_open_batch"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.Fr.ntt)
