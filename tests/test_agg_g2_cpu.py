"""CPU gate of the G2 aggregation layer (include/zkp_bls_agg_g2.h): the planning header under sanitizers at the ABI maxima, at 0 and 1;
the expansion kernel of AggregateVerify compiled for the host and run as written on exactly allocated buffers against the model
(tests/agg_g2_model.py); the model against itself; the boundary - header, ctypes table, Rust block and C sample agree, every symbol is
exported and refuses a null context, every _dev entry has a replay case -; and the code object's new kernels."""
import ctypes
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import agg_g2_model as a2
import agg_model as am
import bls12_381_model as m
from test_agg_cpu import MALFORMED, SAN, _offsets, _split_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkp_bls_agg_g2.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "bls_agg_g2.rs")
C_SAMPLE = os.path.join(ROOT, "integration", "c", "zkp_bls_agg_g2.c")
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
NEW = ["zkp_g2_segment_sum_batch", "zkp_bls_minsig_fast_aggregate_verify_batch", "zkp_bls_aggregate_verify_batch"]
NEW = NEW + [n + "_dev" for n in NEW]


# ----------------------------------------------------------------------------------------------------------------- the planning header
def test_planner_holds_at_the_abi_limits_at_zero_and_at_one(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "agg_g2_plan_check.cpp"), tmp_path / "agg_g2_plan_check"
    subprocess.check_call(SAN + ["-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ----------------------------------------------------------------------------------------------------------------- the expansion kernel's own text
@pytest.fixture(scope="module")
def expand_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("agg_g2_kernels") / "agg_g2_kernel_host")
    cc = subprocess.run(SAN + ["-Wno-unknown-pragmas", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "agg_g2_kernel_host.cpp")],
                        capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _inputs(n, seed, with_inf):
    rng = random.Random(seed)
    sig = [[rng.randrange(1 << 64) for _ in range(24)] for _ in range(n)]
    rand = [[rng.randrange(1, 1 << 64), rng.randrange(1 << 64)] for _ in range(n)]
    inf = [rng.randrange(2) for _ in range(n)] if with_inf else None
    return sig, rand, inf


def _run_expand(exe, tmp_path, seg_off, n_msg, sig, rand, inf):
    """(x_sig rows, x_rand rows, x_inf, status, the call's word, the validation word) of k_agg_check and k_aggv_expand on the host"""
    n = len(seg_off) - 1
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<3Q", n, n_msg, 0 if inf is None else 1) + struct.pack("<%dQ" % (n + 1), *seg_off) +
                    b"".join(struct.pack("<24Q", *r) for r in sig) + b"".join(struct.pack("<2Q", *r) for r in rand) + bytes(inf or []))
    out = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    raw = fout.read_bytes()
    assert len(raw) == 209 * n_msg + n + 8
    xs = [list(struct.unpack_from("<24Q", raw, 192 * i)) for i in range(n_msg)]
    xr = [list(struct.unpack_from("<2Q", raw, 192 * n_msg + 16 * i)) for i in range(n_msg)]
    at = 208 * n_msg
    return xs, xr, list(raw[at:at + n_msg]), list(raw[at + n_msg:at + n_msg + n]), int.from_bytes(raw[-8:-4], "little"), int.from_bytes(raw[-4:], "little")


def _want(seg_off, n_msg, sig, rand, inf):
    n = len(seg_off) - 1
    seg, first, word = a2.expansion(list(seg_off), n_msg, n)
    ident = [0] * 12 + [1] + [0] * 11
    xs = [ident if f is None else sig[f] for f in first]
    xi = [1 if f is None else (0 if inf is None else inf[f]) for f in first]
    xr = [[1, 0] if j is None else rand[j] for j in seg]
    return xs, xr, xi, [0] * n, word


SHAPES = [(1,), (3, 1, 2), (0, 0, 3, 2), (2, 0, 0, 3), (2, 3, 0, 0), (257,), (1,) * 300, (0,), (0, 0)]


@pytest.mark.parametrize("lens", SHAPES, ids=[str(i) for i in range(len(SHAPES))])
@pytest.mark.parametrize("with_inf", [False, True])
def test_expansion_kernel_on_host_equals_the_model(expand_exe, tmp_path, lens, with_inf):
    """one segment; ragged ones; empty segments first, in the middle and last; 257 messages in one segment (two workgroups of lanes)"""
    off = _offsets(lens)
    sig, rand, inf = _inputs(len(lens), len(lens) * 3 + sum(lens), with_inf)
    got = _run_expand(expand_exe, tmp_path, off, off[-1], sig, rand, inf)
    assert got[:5] == _want(off, off[-1], sig, rand, inf) and got[4] == 0 and got[5] == 0


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_expansion_kernel_on_host_follows_no_malformed_offset(expand_exe, tmp_path, kind):
    """both words are set, every message gets the flagged identity and the rand row (1, 0), and (the buffers are exact) nothing outside
    seg_off, sig, inf_sig and rand is touched: a huge offset is never an address"""
    off = MALFORMED[kind]
    sig, rand, inf = _inputs(4, 5, True)
    got = _run_expand(expand_exe, tmp_path, off, 7, sig, rand, inf)
    assert got[:5] == _want(off, 7, sig, rand, inf) and got[4] == 1 and got[5] == 1
    assert got[0] == [[0] * 12 + [1] + [0] * 11] * 7 and got[1] == [[1, 0]] * 7 and got[2] == [1] * 7


@pytest.mark.parametrize("kind", ["decreasing", "first-not-zero", "last-beyond", "last-below"])
def test_expansion_kernel_on_host_follows_no_malformed_offset_of_the_gpu_cases(expand_exe, tmp_path, kind):
    """the four offset lists the GPU tests of the segment sums use (three segments over 45 entries)"""
    from test_gpu_segment_sum import MALFORMED as GPU_MALFORMED
    off = GPU_MALFORMED[kind]
    sig, rand, inf = _inputs(3, 6, False)
    got = _run_expand(expand_exe, tmp_path, off, 45, sig, rand, inf)
    assert got[:5] == _want(off, 45, sig, rand, inf) and got[4] == 1 and got[5] == 1 and got[2] == [1] * 45


def test_expansion_kernel_on_host_with_messages_and_no_signature(expand_exe, tmp_path):
    got = _run_expand(expand_exe, tmp_path, [0], 3, [], [], None)
    assert got[2] == [1, 1, 1] and got[4:] == (1, 1)                       # n == 0 with n_msg > 0 is malformed
    assert _run_expand(expand_exe, tmp_path, [0], 0, [], [], None)[4:] == (0, 0)


# ------------------------------------------------------------------------------------------------------------------- the model against itself
def test_the_expansion_fed_to_plain_bls_verify_is_the_per_segment_definition():
    b = a2.aggregate_verify_batch([2, 1, 2], n_keys=4, seed=3)
    off, n_msg = b["seg_off"], 5
    assert a2.aggregate_verify_model(b["pts"], b["msgs"], off, b["sig_pts"]) == [True, True, True]
    _, first, word = a2.expansion(off, n_msg, 3)
    assert word == 0 and first == [0, None, 1, 2, None]
    expanded = [None if f is None else b["sig_pts"][f] for f in first]
    assert a2.bls_verify_model(b["pts"], b["msgs"], expanded) is True
    # a signature filed under its neighbour: the segments it touches fail
    sigs = [b["sig_pts"][1], b["sig_pts"][0], b["sig_pts"][2]]
    assert a2.aggregate_verify_model(b["pts"], b["msgs"], off, sigs) == [False, False, True]
    # (with every r = 1 the plain product cannot see a swap: that is what distinct rand rows are for, tests/test_gpu_bls_aggregate_verify.py)
    forged = list(b["msgs"])
    forged[3] = b"not the message that was signed"
    assert a2.aggregate_verify_model(b["pts"], forged, off, b["sig_pts"]) == [True, True, False]
    assert a2.bls_verify_model(b["pts"], forged, expanded) is False
    assert a2.aggregate_verify_model(b["pts"], b["msgs"], [0, 2, 2, 3, 5], b["sig_pts"] + [None]) [1] is False     # an empty segment


def test_g2_sums_do_not_depend_on_the_order_of_the_entries():
    pts = a2.g2_table(8)
    rng = random.Random(11)
    idx = [rng.randrange(8) | (am.SIGN if rng.randrange(3) == 0 else 0) for _ in range(12)] + [3, 3 | am.SIGN]
    off = [0, 5, 5, 14]
    want = a2.segment_sums(pts, idx, off)
    for _ in range(3):
        a, b = idx[:5], idx[5:]
        rng.shuffle(a), rng.shuffle(b)
        assert a2.segment_sums(pts, a + b, off) == want
    assert want[0][1] is None and want[1] == [0, 0, 0]
    assert a2.segment_sums(pts, [0, 0 | am.SIGN, 8], [0, 2, 3]) == ([None, None], [0, 1])
    assert a2.segment_sums(pts, [0, 1], [0, 2, 1]) == ([None, None], [1, 1])
    assert a2.segment_sums(pts, [2, 2], [0, 2])[0] == [m.g2_add(pts[2], pts[2])]
    rows, inf, st = a2.sum_rows(pts, idx, off)
    assert rows.shape == (3, 24) and inf.tolist() == [0, 1, 0] and st.tolist() == [0, 0, 0]
    assert rows[1].tolist() == [0] * 12 + [1] + [0] * 11


# ------------------------------------------------------------------------------------------------------------------- the boundary
def _header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _kind_c(t):
    if "*" in t:
        return "ptr"
    if "size_t" in t:
        return "size"
    assert re.search(r"\b(int|unsigned|uint32_t|int32_t)\b", t), t
    return "int"


def _c_signatures(text):
    return {name: (_kind_c(ret), [_kind_c(p) for p in _split_params(params)])
            for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(zkp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


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
    return {name: (kind(ret), [kind(p.split(":", 1)[1]) for p in _split_params(params)])
            for name, params, ret in re.findall(r"pub fn (zkp_[a-z0-9_]+)\s*\(([^)]*)\)\s*->\s*([^;]+);", text)}


def test_header_ctypes_and_rust_agree_and_every_symbol_is_exported():
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    c, rust = _c_signatures(_header_text()), _rust_signatures()
    assert sorted(c) == sorted(NEW) == sorted(_lib.AGG_G2_SIGNATURES) == sorted(rust)
    for name, sig in c.items():
        assert hasattr(lib, name), "libzkp_pairings.so does not export %s" % name
        assert rust[name] == sig, (name, "rust", rust[name], "header", sig)
        if name.endswith("_dev"):
            assert sig[1][-1] == "ptr" and c[name[:-4]] == (sig[0], sig[1][:-1]), name          # the host flavour plus a trailing stream

    def ckind(t):
        if t is ctypes.c_size_t:
            return "size"
        if t in (ctypes.c_int, ctypes.c_uint, ctypes.c_uint32):
            return "int"
        assert t is ctypes.c_void_p, t
        return "ptr"
    for name, (res, args) in _lib.AGG_G2_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args
    tables = [_lib.SIGNATURES, _lib.POLY_SIGNATURES, _lib.PROVE_SIGNATURES, _lib.FK20_SIGNATURES, _lib.CELLS_SIGNATURES, _lib.RECOVER_SIGNATURES,
              _lib.BLS_SIGNATURES, _lib.AGG_SIGNATURES, _lib.GRP_SIGNATURES, _lib.BLS_MINSIG_SIGNATURES, _lib.AGG_G2_SIGNATURES]
    assert sum(len(t) for t in tables) == len(set().union(*tables))                             # the tables are disjoint
    assert lib.zkp_abi_version() == 4
    # the G1 twins' argument lists carry over: the sums to the letter, the committee verifier to the letter
    assert _lib.AGG_G2_SIGNATURES["zkp_g2_segment_sum_batch"] == _lib.AGG_SIGNATURES["zkp_g1_segment_sum_batch"]
    assert _lib.AGG_G2_SIGNATURES["zkp_bls_minsig_fast_aggregate_verify_batch_dev"] == _lib.AGG_SIGNATURES["zkp_bls_fast_aggregate_verify_batch_dev"]


def test_the_c_sample_names_the_same_symbols_with_the_same_argument_counts_and_links(tmp_path):
    c = _c_signatures(_header_text())
    with open(C_SAMPLE) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    host = [n for n in NEW if not n.endswith("_dev")]
    for name in host:
        calls = re.findall(r"\b%s\(((?:[^()]|\([^()]*\))*)\)" % name, text)
        assert calls, name
        for args in calls:
            depth, count = 0, 1
            for ch in args:
                depth += ch == "("
                depth -= ch == ")"
                count += ch == "," and depth == 0
            assert count == len(c[name][1]), (name, count)
    so = os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    exe = tmp_path / "zkp_bls_agg_g2"
    cc = subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), C_SAMPLE, "-L", os.path.dirname(so), "-lzkp_pairings",
                         "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined", "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]


def test_the_old_boundary_gained_one_module_line_and_the_new_header_its_sections():
    names = "|".join(n for n in NEW if not n.endswith("_dev"))
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "zkp_bls_agg_g2.h":
            with open(os.path.join(ROOT, "include", other)) as f:
                assert not re.search(names, f.read()), other
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert len(re.findall(r"^(?:pub )?mod bls_agg_g2;$", lib_rs, re.M)) == 1 and not re.search(names, lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_bls_agg_g2.hip", "zkp_bls_agg_g2.hpp", "zkp_bls_agg_g2_plan.hpp", "include/zkp_bls_agg_g2.h"))
    with open(HEADER) as f:
        text = f.read()
    assert all(x in text for x in ('#include "zkp_bls.h"', "under ABI version 4", "Slices and workspace", "Cost:", "How", "ZKP_ERR_ARG", "Out of scope",
                                   "distinctness", "table_inf", "4 GB"))
    for older in ("zkp_bls_agg.h", "zkp_bls_grouped.h", "zkp_bls_minsig.h"):
        with open(os.path.join(ROOT, "include", older)) as f:
            assert "zkp_bls_agg_g2.h" in f.read(), older
    # zkp_coop.hip and the index kernels are used as they are: the new unit brings no copy of the accumulation, of the check or of the search's keys
    with open(os.path.join(CSRC, "zkp_bls_agg_g2.hip")) as f:
        unit = f.read()
    assert "msm_accum(2, lv == 0" in unit and "msm_points(" in unit and "hipMemsetAsync" not in unit and "jac_madd" not in unit
    assert "aggk::check(" in unit and "aggk::keys(" in unit and "aggk::fold(" in unit and "__global__ void __launch_bounds__(TPB_I)" not in unit
    assert "minsig_verify_dev(" in unit and "bls_verify_dev(" in unit and "coop_pairing" not in unit          # no second pairing path


def test_every_dev_entry_point_has_a_replay_case_or_a_written_reason():
    import agg_g2_replay_cases as arc
    declared = set(re.findall(r"\b(zkp_\w+_dev)\(", _header_text()))
    table, excluded = arc.table_c_names(), set(arc.EXCLUDED)
    assert declared == {n for n in NEW if n.endswith("_dev")}
    assert not (table & excluded)
    assert declared - (table | excluded) == set(), "no replay case and no reason: %s" % sorted(declared - (table | excluded))
    assert (table | excluded) - declared == set()
    assert all(isinstance(why, str) and len(why) > 20 for why in arc.EXCLUDED.values())
    from zkvm_pairings_amd.engine import PairingEngine
    for c in arc.CASES:
        assert callable(getattr(PairingEngine, c.method)), c.id


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    for name, (_, args) in _lib.AGG_G2_SIGNATURES.items():
        assert getattr(lib, name)(*[None if a is ctypes.c_void_p else 0 for a in args]) == -1, name
    for name in ("g2_segment_sum", "bls_minsig_fast_aggregate_verify", "bls_aggregate_verify"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("bls_aggregate_signatures", "bls_minsig_aggregate_keys", "bls_minsig_fast_aggregate_verify_batch", "bls_minsig_fast_aggregate_verify_each",
                 "bls_aggregate_verify_batch", "bls_aggregate_verify_each"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.synthetic.bls_minsig_aggregate_instance) and callable(z.synthetic.bls_aggregate_verify_instance)


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_are_there_and_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_agg2_" in n or "k_aggv_" in n}
    for part in ("k_agg2_affine", "k_aggv_expand"):
        assert sum(part in n for n in new) == 1, part
    assert len(new) == 2, sorted(new)
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)
    assert [v["lds"] for n, v in new.items() if "k_agg2_affine" in n] == [8192]         # two planes of 64 values: prefix and suffix products
    assert [v["vgpr"] <= 256 for n, v in new.items() if "k_agg2_affine" in n] == [True]
    assert len([n for n in k if "k_agg_" in n]) == 5                                    # the index kernels are not compiled a second time


def test_the_timing_tool_parses_its_arguments_and_names_engine_methods_that_exist():
    tool = os.path.join(ROOT, "tools", "time_agg_g2.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--shapes" in out.stdout and "--verify-shapes" in out.stdout and "--table" in out.stdout
    from zkvm_pairings_amd.engine import PairingEngine
    with open(tool) as f:
        text = f.read()
    used = set(re.findall(r"\beng\.([a-z_0-9]+)\(", text))
    assert {"g2_segment_sum", "bls_minsig_fast_aggregate_verify", "bls_aggregate_verify", "g2_add", "bls_minsig_verify", "bls_verify"} <= used
    for name in used:
        assert callable(getattr(PairingEngine, name)), name
