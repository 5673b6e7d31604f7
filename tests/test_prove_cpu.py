"""CPU gate for the Groth16 producer side (include/zkp_prove.h): the Python model of the quotient against schoolbook division and the
proof exponents against the verification equation; the planner (csrc/zkp_prove_plan.hpp) walked to the ABI maxima under ASan and UBSan
(tests/prove_plan_check.cpp, a child process) and its lane counts over the shape table of the GPU tests; the kernels' own text on host
threads (tests/prove_kernel_host.cpp) against the model, a malformed matrix among the inputs; the new header, the ctypes table and the
Rust file against one another; the replay table against the header; the new kernels' registers."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import poly_model as pm
import prove_model as pmod
import prove_shapes as ps
from replay_cases import fr_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "zkp_prove.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "prove.rs")
R = pm.R
NEW = ["zkp_fr_spmv_batch", "zkp_fr_spmv_batch_dev", "zkp_groth16_quotient_batch", "zkp_groth16_quotient_batch_dev", "zkp_groth16_prove_batch",
       "zkp_groth16_prove_batch_dev"]


def _secrets(*a, **k):
    from zkvm_pairings_amd import synthetic
    return synthetic.groth16_circuit_secrets(*a, **k)


# ------------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("log2_n", range(1, 7))
def test_model_quotient_against_schoolbook_division(log2_n):
    """h of the coset formula is (a b - c) / (X^N - 1) with remainder zero for a satisfying witness, of degree <= N - 2; for a witness
    that violates a row the division leaves a remainder and sat is 0"""
    n = 1 << log2_n
    for n_rows in sorted(set((n, n - 1, 1))):
        s = _secrets(0x51 + log2_n, log2_n, n_rows, n + 3, 1, 2, bad=(1,))
        for j, z in enumerate(s["z"]):
            a, b, c = (pm.ntt(v, log2_n, inverse=True) for v in pmod.evaluations(s, z))
            p = pmod.poly_mul(a, b)
            for i, v in enumerate(c):
                p[i] = (p[i] - v) % R
            quo, rem = pmod.divide_by_vanishing(p, n)
            h, sat = pmod.quotient(s, z)
            assert sat == (j == 0) and sat == (not any(rem)), (log2_n, n_rows, j)
            if sat:
                assert h == quo + [0] * (n - len(quo)) and h[n - 1] == 0, (log2_n, n_rows)
            else:
                assert h != quo + [0] * (n - len(quo))
            # the defining property, for either kind of witness: h on the coset
            kinv = pow(pow(7, n, R) - 1, -1, R)
            x = 7 * pm.root_of_unity(log2_n) % R
            assert pmod.horner(h, x) == (pmod.horner(a, x) * pmod.horner(b, x) - pmod.horner(c, x)) * kinv % R


@pytest.mark.parametrize("log2_n,n_inputs", [(1, 0), (2, 1), (3, 5), (5, 2)])
def test_proof_exponents_satisfy_the_verification_equation(log2_n, n_inputs):
    n = 1 << log2_n
    s = _secrets(0x77 + log2_n, log2_n, n, n + 3, n_inputs, 3, bad=(1,))
    rng = random.Random(log2_n)
    for j, z in enumerate(s["z"]):
        for r, t in ((rng.randrange(R), rng.randrange(R)), (0, 0)):
            e_a, e_b, e_c = pmod.proof_exponents(s, z, r, t)
            assert pmod.verifies(s, z, e_a, e_b, e_c) == (j != 1), (log2_n, j)
            if j != 1:       # h(tau) of the H sum is (a b - c)(tau) / t(tau)
                a_t, b_t, c_t = pmod.at_tau(s, z)
                h, _ = pmod.quotient(s, z)
                assert pmod.horner(h[:n - 1], s["tau"]) == (a_t * b_t - c_t) * pow(pow(s["tau"], n, R) - 1, -1, R) % R
    # the QAP polynomials at tau are what the definitions say: u_i(tau) = sum_k A[k][i] l_k(tau), through the evaluations of a witness
    z = s["z"][0]
    a_ev = pmod.evaluations(s, z)[0]
    assert pmod.horner(pm.ntt(a_ev, log2_n, inverse=True), s["tau"]) == pmod.at_tau(s, z)[0]


def test_builder_makes_what_it_promises():
    s = _secrets(3, 3, 7, 11, 2, 4, bad=(2,))
    assert len(s["z"]) == 4 and all(len(z) == 11 and z[0] == 1 for z in s["z"])
    assert [pmod.quotient(s, z)[1] for z in s["z"]] == [True, True, False, True]
    assert s["u_tau"][10] == 0 and s["v_tau"][10] == 0 and s["w_tau"][10] != 0        # the last product variable: an infinite query entry
    assert all(len(row) == 1 and row[0] == (11 - 7 + k, 1) for k, row in enumerate(s["rows_c"]))
    assert {c for c, _ in s["rows_a"][0] + s["rows_a"][1] + s["rows_a"][2]} >= {0, 1, 2}
    s2 = _secrets(3, 3, 7, 11, 2, 1, row_lengths=[4] * 7)
    assert all(len(a) == 4 and len(b) == 4 for a, b in zip(s2["rows_a"], s2["rows_b"]))


# ------------------------------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prove_plan") / "prove_plan_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         "-o", exe, os.path.join(ROOT, "tests", "prove_plan_check.cpp")], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _clean(out):
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]


def test_planner_holds_at_the_abi_maxima(plan_exe):
    out = subprocess.run([plan_exe], capture_output=True, text=True, timeout=900)
    _clean(out)
    assert re.search(r"prove plan_check ok: \d+ cases", out.stdout)
    for src in ("zkp_prove.hip", "zkp_pairings.hip"):
        with open(os.path.join(CSRC, src)) as f:
            assert '#include "zkp_prove_plan.hpp"' in f.read()


def test_shape_table_hits_every_lane_count(plan_exe):
    """the planner's own t for every matrix of tests/prove_shapes.py: all of 0 .. 6, and what the table's comment expects"""
    names = [n for n in ps.SPMV if ps.SPMV[n][0]]
    args = []
    for n in names:
        lengths = ps.SPMV[n][0]
        args += [str(sum(lengths)), str(len(lengths))]
    out = subprocess.run([plan_exe, "t"] + args, capture_output=True, text=True, timeout=900)
    _clean(out)
    got = [int(x) for x in out.stdout.split()]
    assert got == [ps.expected_t(ps.SPMV[n][0]) for n in names]
    assert set(got) == set(range(7)), dict(zip(names, got))
    assert dict(zip(names, got))["mixed"] == 6


# ------------------------------------------------------------------------------------------------------------------- the kernels' own text
@pytest.fixture(scope="module")
def kernel_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prove_kernels") / "prove_kernel_host")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                         "-Wno-unknown-pragmas", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "prove_kernel_host.cpp")], capture_output=True, text=True,
                        timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _kernel_run(exe, args):
    _clean(subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=900))


def _spmv_input(rows, xs, row_ptr=None, col=None):
    rp, cl, val = ps.csr(rows)
    rp = rp if row_ptr is None else np.array(row_ptr, dtype=np.uint32)
    cl = cl if col is None else np.array(col, dtype=np.uint32)
    return rp.tobytes() + cl.tobytes() + val.tobytes() + fr_rows([v for x in xs for v in x]).tobytes()


@pytest.mark.parametrize("name", list(ps.SPMV))
def test_spmv_kernel_on_host_threads_equals_the_model(kernel_exe, tmp_path, name):
    """k_spmv as written, at the planner's lane count and, for the mixed matrix, at every other one (the bytes do not depend on t);
    the padding up to out_stride is zero on an output pre-filled with ones; the flag stays clear"""
    rows, n_cols = ps.spmv_matrix(name)
    nnz = sum(len(r) for r in rows)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    for n in ps.SPMV_N:
        xs = ps.spmv_vectors(name, n)
        fin.write_bytes(_spmv_input(rows, xs))
        for out_stride in (len(rows), len(rows) + 3):
            want = ps.spmv_expected(rows, xs, out_stride).tobytes() + b"\0\0\0\0"
            for t in ([-1] + list(range(7)) if name == "mixed" and n == 3 else [-1]):
                _kernel_run(kernel_exe, ["spmv", fin, fout, len(rows), n_cols, nnz, n, out_stride, t, 0])
                assert fout.read_bytes() == want, (name, n, out_stride, t)


def test_spmv_kernel_stores_bit_reversed_for_the_quotient(kernel_exe, tmp_path):
    rows, n_cols = ps.spmv_matrix("len3")
    rows = rows[:29]
    xs = ps.spmv_vectors("len3", 3)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(_spmv_input(rows, xs))
    _kernel_run(kernel_exe, ["spmv", fin, fout, len(rows), n_cols, sum(len(r) for r in rows), 3, 32, -1, 5])
    nat = ps.spmv_expected(rows, xs, 32)
    want = np.stack([nat[j][[pm.bit_reverse(i, 5) for i in range(32)]] for j in range(3)])
    assert fout.read_bytes() == want.tobytes() + b"\0\0\0\0"


def test_spmv_kernel_never_reads_outside_a_malformed_matrix(kernel_exe, tmp_path):
    """a column >= n_cols, a row bound beyond nnz and a decreasing row bound: the sanitizers stay silent (every array has exactly its
    promised size), the offending entries contribute nothing, the flag is set"""
    rows, n_cols = ps.spmv_matrix("len7")
    rows = rows[:20]
    xs = ps.spmv_vectors("len7", 3)
    rp, cl, _ = ps.csr(rows)
    nnz = int(rp[-1])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    # (a) columns out of range: n_cols itself, and the largest 32-bit value
    col = cl.copy()
    col[3], col[50] = n_cols, 0xFFFFFFFF
    kept = [[(c, v) for i, (c, v) in enumerate(row) if 7 * k + i not in (3, 50)] for k, row in enumerate(rows)]
    fin.write_bytes(_spmv_input(rows, xs, col=col))
    _kernel_run(kernel_exe, ["spmv", fin, fout, len(rows), n_cols, nnz, 3, 20, -1, 0])
    assert fout.read_bytes() == ps.spmv_expected(kept, xs, 20).tobytes() + b"\1\0\0\0"
    # (b) row bounds: the last one far beyond nnz, one in the middle beyond nnz, one decreasing
    for which, value in ((20, 0xFFFFFFF0), (10, nnz + 5), (5, 7)):
        bad = rp.copy()
        bad[which] = value
        lo = [min(int(bad[k]), nnz) for k in range(20)]
        hi = [min(int(bad[k + 1]), nnz) for k in range(20)]
        flat = [e for row in rows for e in row]
        kept = [flat[min(lo[k], hi[k]):hi[k]] for k in range(20)]
        fin.write_bytes(_spmv_input(rows, xs, row_ptr=bad))
        for t in (-1, 0, 6):
            _kernel_run(kernel_exe, ["spmv", fin, fout, len(rows), n_cols, nnz, 3, 20, t, 0])
            assert fout.read_bytes() == ps.spmv_expected(kept, xs, 20).tobytes() + b"\1\0\0\0", (which, t)


@pytest.mark.parametrize("log2_n,n", [(1, 3), (3, 3), (8, 2), (9, 1)])
def test_quotient_and_satisfaction_kernels_on_host_threads(kernel_exe, tmp_path, log2_n, n):
    rng = random.Random(0x9A + log2_n)
    big_n = 1 << log2_n
    a = [rng.randrange(R) for _ in range(n * big_n)]
    b = [rng.randrange(R) for _ in range(n * big_n)]
    c = [x * y % R for x, y in zip(a, b)]
    a[0], b[0], c[0] = R - 1, R - 1, 1
    sat = [1] * n
    if n > 1:
        c[big_n + big_n // 2] = (c[big_n + big_n // 2] + 1) % R          # witness 1 violates one slot
        sat[1] = 0
    kinv = pow(pow(7, big_n, R) - 1, -1, R)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(pm.to_bytes(a) + pm.to_bytes(b) + pm.to_bytes(c))
    _kernel_run(kernel_exe, ["quot", fin, fout, log2_n, n])
    assert fout.read_bytes() == bytes(sat) + pm.to_bytes([(x * y - w) * kinv % R for x, y, w in zip(a, b, c)])


def test_assembly_kernels_on_host_threads(kernel_exe, tmp_path):
    rng = random.Random(0xA55)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    n = 300
    rs = [(rng.randrange(R), rng.randrange(R)) for _ in range(n)]
    rs[0], rs[1], rs[2] = (0, 0), (R - 1, R - 1), (0, 5)
    fin.write_bytes(pm.to_bytes([v for p in rs for v in p]))
    _kernel_run(kernel_exe, ["rs", fin, fout, n])
    assert fout.read_bytes() == pm.to_bytes([r for r, _ in rs]) + pm.to_bytes([s for _, s in rs]) + pm.to_bytes([-r * s % R for r, s in rs])
    inf_pt = np.zeros(12, dtype=np.uint64)
    inf_pt[6] = 1
    for n_src, lead, total, with_inf in ((5, 3, 8, 1), (300, 2, 302, 0), (0, 4, 4, 0), (7, 0, 8, 1)):
        src = np.arange(1, 12 * n_src + 1, dtype=np.uint64).reshape(n_src, 12)
        inf = np.array([(i % 3 == 1) * 5 for i in range(n_src)], dtype=np.uint8)
        fin.write_bytes(src.tobytes() + (inf.tobytes() if with_inf else b""))
        _kernel_run(kernel_exe, ["pad", fin, fout, n_src, lead, total, with_inf])
        dst = np.tile(inf_pt, (total, 1))
        dinf = np.ones(total, dtype=np.uint8)
        for i in range(n_src):
            if not (with_inf and inf[i]):
                dst[lead + i], dinf[lead + i] = src[i], 0
        assert fout.read_bytes() == dst.tobytes() + dinf.tobytes(), (n_src, lead, total)
    pt = np.arange(7, 31, dtype=np.uint64)
    fin.write_bytes(pt.tobytes())
    _kernel_run(kernel_exe, ["bcast", fin, fout, 24, 11])
    assert fout.read_bytes() == np.tile(pt, 11).tobytes()
    base_inf = np.array([0, 1, 0, 0, 9] * 60, dtype=np.uint8)
    out = np.arange(12 * 300, dtype=np.uint64).reshape(300, 12)
    oinf = np.zeros(300, dtype=np.uint8)
    fin.write_bytes(base_inf.tobytes() + out.tobytes() + oinf.tobytes())
    _kernel_run(kernel_exe, ["mulinf", fin, fout, 300])
    out[base_inf != 0], oinf[base_inf != 0] = inf_pt, 1
    assert fout.read_bytes() == out.tobytes() + oinf.tobytes()


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


def _rust_text():
    with open(RUST) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def _rust_signatures():
    def kind(t):
        t = t.strip()
        if t.startswith("*"):
            return "ptr"
        if t == "usize":
            return "size"
        assert t in ("c_int", "c_uint", "u32", "i32"), t
        return "int"
    out = {}
    for name, params, ret in re.findall(r"pub fn (zkp_[a-z0-9_]+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", _rust_text()):
        out[name] = ("void" if not ret.strip() else kind(ret), [kind(p.split(":", 1)[1]) for p in _split_params(params)])
    return out


def _c_struct_fields(name):
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, _header_text()).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(const void|size_t|unsigned|zkp_fr_csr)\b", decl).group(1)
        for item in decl[len(base):].split(","):
            item = item.strip()
            fields.append((item.lstrip("*"), "ptr" if item.startswith("*") else {"size_t": "size", "unsigned": "int", "zkp_fr_csr": "csr"}[base]))
    return fields


def _rust_struct_fields(name):
    body = re.search(r"pub struct %s \{([^{}]*)\}" % name, _rust_text()).group(1)
    kinds = {"usize": "size", "c_uint": "int", "ZkpFrCsr": "csr"}
    return [(f.strip(), "ptr" if t.strip().startswith("*") else kinds[t.strip()])
            for f, t in (x.replace("pub ", "").split(":") for x in body.split(",") if x.strip())]


def test_header_ctypes_and_rust_agree_and_every_symbol_is_exported():
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    names = _declared_symbols()
    assert names == sorted(NEW)
    c = _c_signatures()
    assert sorted(c) == names and sorted(_lib.PROVE_SIGNATURES) == names
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
    for name, (res, args) in _lib.PROVE_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args                                   # load() bound the third table as well
    assert not set(_lib.PROVE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.POLY_SIGNATURES))
    assert lib.zkp_abi_version() == 4
    # the three descriptors: header, ctypes, Rust - the same fields in the same order
    def pykind(t):
        return "csr" if t is _lib.FrCsr else ckind(t)
    for cname, cls, rname in (("zkp_fr_csr", _lib.FrCsr, "ZkpFrCsr"), ("zkp_r1cs", _lib.R1cs, "ZkpR1cs"), ("zkp_groth16_pk", _lib.Groth16Pk, "ZkpGroth16Pk")):
        want = _c_struct_fields(cname)
        assert [(f, pykind(t)) for f, t in cls._fields_] == want, cname
        assert _rust_struct_fields(rname) == want, rname


def test_the_old_boundary_gained_one_comment_and_one_module_line():
    with open(os.path.join(ROOT, "include", "zkp_pairings.h")) as f:
        old = f.read()
    assert "zkp_prove.h" in old and not any(n + "(" in old for n in NEW) and not re.search(r"zkp_(fr_spmv|groth16_quotient|groth16_prove)", old)
    with open(os.path.join(ROOT, "include", "zkp_poly.h")) as f:
        assert not re.search(r"zkp_(fr_spmv|groth16_quotient|groth16_prove)", f.read())
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert re.search(r"^(pub )?mod prove;$", lib_rs, re.M) and not re.search(r"zkp_(fr_spmv|groth16_quotient|groth16_prove)", lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_prove.hip", "zkp_prove.hpp", "zkp_prove_plan.hpp", "include/zkp_prove.h"))
    with open(HEADER) as f:
        h = f.read()
    assert all(x in h for x in ("zkp_g1_is_valid_batch", "TRUSTED", "input-consistency", "under ABI version 4", "UNIFORMLY", "Slices and workspace"))


def test_every_dev_entry_point_of_the_new_header_has_a_replay_case_or_a_written_reason():
    import prove_replay_cases as prc
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
    assert {c.method: (c.shape, c.small) for c in prc.CASES} == {m: ((3, 6), (1, 2)) for m in ("fr_spmv", "groth16_quotient", "groth16_prove")}   # N = 64, N = 4


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_spmv" in n or "k_prove_" in n}
    assert len(new) == 1 + 7, sorted(new)             # the product; sat_init, sat, quot, rs, pad, bcast, mulinf
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)
        assert v["vgpr"] <= 128, (n, v)               # four waves per SIMD: the gathers have something to hide behind
    spmv = [v for n, v in new.items() if "k_spmv" in n][0]
    assert spmv["lds"] == 8 * 256 * 4, spmv           # the lane sums: eight words per lane
    old = {n for n in k if any(x in n for x in ("k_coop", "k_ntt_pass", "k_poly_coset", "k_open_quot"))}
    assert not (old & set(new))


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    assert lib.zkp_fr_spmv_batch(None, None, None, 0, 0, None) == -1 and lib.zkp_fr_spmv_batch_dev(None, None, None, 0, 0, None, None) == -1
    assert lib.zkp_groth16_quotient_batch(None, None, None, 0, None, None) == -1
    assert lib.zkp_groth16_quotient_batch_dev(None, None, None, 0, None, None, None) == -1
    assert lib.zkp_groth16_prove_batch(None, None, None, None, None, 0, 0, None, None, None, None, None, None, None) == -1
    assert lib.zkp_groth16_prove_batch_dev(None, None, None, None, None, 0, 0, None, None, None, None, None, None, None, None) == -1
    for name in ("fr_spmv", "groth16_quotient", "groth16_prove"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("R1CS", "Groth16ProvingKey", "groth16_prove_batch", "groth16_quotient_batch"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.synthetic.groth16_circuit_instance)
