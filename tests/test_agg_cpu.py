"""CPU gate of the committee aggregation layer (include/zkp_bls_agg.h): the planning header under sanitizers at the ABI maxima and around
every power of the run length, the index kernels compiled for the host and run as written on exactly allocated buffers against the model
(tests/agg_model.py), the boundary - header, ctypes table and Rust block agree, every symbol is exported and refuses a null context, every
_dev entry has a replay case -, the code object's k_agg_* set, and the Python helpers against the model."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import agg_model as am
import bls12_381_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkp_bls_agg.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "bls_agg.rs")
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
NEW = ["zkp_g1_segment_sum_batch", "zkp_bls_fast_aggregate_verify_batch"]
NEW = NEW + [n + "_dev" for n in NEW]
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror"]


# ----------------------------------------------------------------------------------------------------------------- the planning header
def test_planner_holds_at_the_abi_limits_and_around_every_power_of_the_run(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "agg_plan_check.cpp"), tmp_path / "agg_plan_check"
    subprocess.check_call(SAN + ["-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ----------------------------------------------------------------------------------------------------------------- the index kernels' own text
@pytest.fixture(scope="module")
def index_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("agg_kernels") / "agg_kernel_host")
    cc = subprocess.run(SAN + ["-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "agg_kernel_host.cpp")], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _run_index(exe, tmp_path, n_table, idx, seg_off):
    """(keys, vals, status, the call's word, the validation word) of k_agg_check and k_agg_keys on host"""
    n_idx, n_seg = len(idx), len(seg_off) - 1
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<3Q", n_table, n_idx, n_seg) + struct.pack("<%dI" % n_idx, *idx) + struct.pack("<%dQ" % (n_seg + 1), *seg_off))
    out = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    raw = fout.read_bytes()
    assert len(raw) == 8 * n_idx + n_seg + 8
    keys = list(struct.unpack_from("<%dI" % n_idx, raw, 0))
    vals = list(struct.unpack_from("<%dI" % n_idx, raw, 4 * n_idx))
    return keys, vals, list(raw[8 * n_idx:8 * n_idx + n_seg]), int.from_bytes(raw[-8:-4], "little"), int.from_bytes(raw[-4:], "little")


def _offsets(lens):
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    return off


def _entries(n, n_table, seed):
    import random
    rng = random.Random(seed)
    return [rng.randrange(n_table) | (am.SIGN if rng.randrange(3) == 0 else 0) for _ in range(n)]


WELL_FORMED = [(0, 0, 3, 0, 0, 1, 2, 0), (5,), (0,), (0, 0), (1, 31, 1, 32, 33, 0, 64, 0, 0, 2), (1,) * 300, (700, 0, 1)]


@pytest.mark.parametrize("lens", WELL_FORMED, ids=[str(i) for i in range(len(WELL_FORMED))])
def test_index_kernels_on_host_equal_the_model_on_well_formed_entries(index_exe, tmp_path, lens):
    """empty segments first, last and next to each other; more than one workgroup of entries and of offsets"""
    off = _offsets(lens)
    idx = _entries(off[-1], 37, len(lens))
    keys, vals, status, word, bad = _run_index(index_exe, tmp_path, 37, idx, off)
    assert (keys, vals, status, word) == am.keys_values(idx, off, 37) and bad == 0
    assert keys == sorted(keys) and all(off[k] <= e < off[k + 1] for e, k in enumerate(keys))


def test_index_kernels_on_host_mark_rows_beyond_the_table_and_never_use_them(index_exe, tmp_path):
    off = _offsets((2, 3, 0, 4, 1))
    idx = _entries(10, 37, 9)
    idx[3] = 37                                      # the first row that does not exist
    idx[9] = 0x7FFFFFFF                              # the largest row an entry can name
    idx[5] = 36 | am.SIGN                            # the last row, subtracted: sound
    keys, vals, status, word, bad = _run_index(index_exe, tmp_path, 37, idx, off)
    assert (keys, vals, status, word) == am.keys_values(idx, off, 37) and (word, bad) == (0, 0)
    assert status == [0, 1, 0, 0, 1] and vals[3] == 0 and vals[9] == 0 and vals[5] == idx[5]
    idx[9] = 0xFFFFFFFF                              # ... with the sign: the sign survives, the row becomes 0
    keys, vals, status, word, _ = _run_index(index_exe, tmp_path, 37, idx, off)
    assert vals[9] == am.SIGN and status[4] == 1 and all(v & am.ROW < 37 for v in vals)


MALFORMED = {"decreasing": [0, 4, 3, 7, 7], "first-not-zero": [1, 4, 5, 7, 7], "last-beyond": [0, 4, 5, 7, 8], "last-below": [0, 4, 5, 6, 6],
             "decreasing-far": [0, 1 << 50, 3, 7, 7], "all-huge": [1 << 60, 1 << 61, 1 << 62, 1 << 63, 7]}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_index_kernels_on_host_follow_no_malformed_offset(index_exe, tmp_path, kind):
    """every key is KEY_NONE, both words are set, and (the buffers are exact) nothing outside idx, seg_off and status is touched"""
    off = MALFORMED[kind]
    idx = _entries(7, 37, 3)
    keys, vals, status, word, bad = _run_index(index_exe, tmp_path, 37, idx, off)
    assert (keys, vals, status, word) == am.keys_values(idx, off, 37) and word == 1 and bad == 1
    assert keys == [am.KEY_NONE] * 7 and status == [0] * 4        # k_agg_affine turns the word into every status


def test_index_kernels_on_host_with_no_segment_and_with_no_entry(index_exe, tmp_path):
    assert _run_index(index_exe, tmp_path, 37, [], [0]) == ([], [], [], 0, 0)
    assert _run_index(index_exe, tmp_path, 0, [], [0, 0, 0]) == ([], [], [0, 0], 0, 0)
    keys, _, _, word, bad = _run_index(index_exe, tmp_path, 37, [1, 2], [0])          # entries and no segment to hold them
    assert keys == [am.KEY_NONE] * 2 and (word, bad) == (1, 1)


# ------------------------------------------------------------------------------------------------------------------- the boundary
def _header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _split_params(txt):
    txt = txt.strip()
    return [] if txt in ("", "void") else [p.strip() for p in txt.split(",")]


def _c_signatures():
    def kind(t):
        if "*" in t:
            return "ptr"
        if "size_t" in t:
            return "size"
        if re.search(r"\b(int|unsigned|uint32_t|int32_t)\b", t):
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
    c = _c_signatures()
    assert sorted(c) == sorted(NEW) == sorted(_lib.AGG_SIGNATURES)
    rust = _rust_signatures()
    assert sorted(rust) == sorted(NEW)
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
    for name, (res, args) in _lib.AGG_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args
    tables = [_lib.SIGNATURES, _lib.POLY_SIGNATURES, _lib.PROVE_SIGNATURES, _lib.FK20_SIGNATURES, _lib.CELLS_SIGNATURES, _lib.RECOVER_SIGNATURES,
              _lib.BLS_SIGNATURES, _lib.AGG_SIGNATURES]
    assert sum(len(t) for t in tables) == len(set().union(*tables))
    assert lib.zkp_abi_version() == 4


def test_the_old_boundary_gained_one_module_line():
    names = "|".join(n for n in NEW if not n.endswith("_dev"))
    for other in ("zkp_pairings.h", "zkp_poly.h", "zkp_prove.h", "zkp_fk20.h", "zkp_cells.h", "zkp_recover.h", "zkp_bls.h"):
        with open(os.path.join(ROOT, "include", other)) as f:
            assert not re.search(names, f.read()), other
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert len(re.findall(r"^(?:pub )?mod bls_agg;$", lib_rs, re.M)) == 1 and not re.search(names, lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_bls_agg.hip", "zkp_bls_agg.hpp", "zkp_bls_agg_plan.hpp", "include/zkp_bls_agg.h"))
    assert os.path.exists(os.path.join(ROOT, "integration", "c", "zkp_bls_agg.c"))
    with open(HEADER) as f:
        text = f.read()
    assert all(x in text for x in ('#include "zkp_bls.h"', "under ABI version 4", "Slices and workspace", "Cost:", "How", "ZKP_ERR_ARG", "Out of scope"))
    # zkp_coop.hip, whose kernels' registers other gates pin, is used as it is: the new unit brings no copy of its accumulation
    with open(os.path.join(CSRC, "zkp_bls_agg.hip")) as f:
        unit = f.read()
    assert "msm_accum(1, lv == 0" in unit and "msm_points(" in unit and "hipMemsetAsync" not in unit and "jac_madd" not in unit


def test_every_dev_entry_point_has_a_replay_case_or_a_written_reason():
    import agg_replay_cases as arc
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
        assert c.shape[1] > 32 >= c.small[1], c.id                   # two accumulation levels under capture, one in the smaller call


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    for name, (_, args) in _lib.AGG_SIGNATURES.items():
        assert getattr(lib, name)(*[None if a is ctypes.c_void_p else 0 for a in args]) == -1, name
    for name in ("g1_segment_sum", "bls_fast_aggregate_verify"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("committee_entries", "bls_aggregate_keys", "bls_fast_aggregate_verify_batch", "bls_fast_aggregate_verify_each"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.synthetic.bls_aggregate_instance)


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_are_there_and_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_agg_" in n}
    for part in ("k_agg_zero", "k_agg_check", "k_agg_keys", "k_agg_affine", "k_agg_fold"):
        assert sum(part in n for n in new) == 1, part
    assert len(new) == 5, sorted(new)
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)
    assert [v["lds"] for n, v in new.items() if "k_agg_affine" in n] == [8192]          # two planes of 64 values: prefix and suffix products
    counted = ("k_ntt_pass", "k_msm_", "k_add28", "k_g1_mul_endo28", "k_fr_", "k_kzg_", "k_prove_", "k_spmv", "k_poly_coset", "k_open_quot", "k_rlc_",
               "k_g16_", "k_frinv_", "k_freval_", "k_zero_fill", "k_coop", "k_g1ntt_", "k_fk20_", "k_cell_", "k_rec_", "k_h2", "k_bls_")
    assert not [n for n in new for x in counted if x in n]


# ------------------------------------------------------------------------------------------------------------------- the Python helpers
def test_committee_entries_equals_the_model_in_its_three_forms():
    import zkvm_pairings_amd as z
    committees = [[3, 1, 4], [], [1, 5, 9, 2, 6], [5], []]
    bits = [[1, 0, 1], [], [0, 0, 0, 0, 0], [1], []]
    for kw in (dict(), dict(bits=bits), dict(absent_from=36), dict(absent_from=[36, 35, 34, 33, 32])):
        idx, seg_off = z.committee_entries(committees, **kw)
        want_idx, want_off = am.committee_entries(committees, **kw)
        assert idx.dtype == np.uint32 and seg_off.dtype == np.uint64
        assert idx.tolist() == want_idx and seg_off.tolist() == want_off
        assert am.offsets_sound(seg_off.tolist(), idx.size)
    idx, seg_off = z.committee_entries(committees, absent_from=36)
    assert idx.tolist()[:4] == [36, 3 | am.SIGN, 1 | am.SIGN, 4 | am.SIGN] and seg_off.tolist() == [0, 4, 5, 11, 13, 14]
    assert z.committee_entries([])[0].size == 0 and z.committee_entries([])[1].tolist() == [0]
    for bad in (dict(committees=[[1 << 31]]), dict(committees=[[-1]]), dict(committees=[[1]], bits=[[1, 0]]), dict(committees=[[1]], bits=[[1]], absent_from=0),
                dict(committees=[[1], [2]], absent_from=[3])):
        with pytest.raises(ValueError):
            z.committee_entries(**bad)


def test_the_model_sums_as_the_group_does():
    """tests/agg_model.py itself: signs, doublings, cancellations, empty segments, rows beyond the table, malformed offsets"""
    _, pks = am.key_table(8)
    a, b = pks[0], pks[1]
    idx = [0, 0 | am.SIGN, 0, 0, 0, 1, 0 | am.SIGN, 1 | am.SIGN, 1, 8]
    off = [0, 2, 2, 4, 8, 10]
    pts, st = am.segment_sums(pks, idx, off)
    assert pts == [None, None, m.g1_add(a, a), None, None] and st == [0, 0, 0, 0, 1]
    assert am.segment_sums(pks, [0, 1], [0, 1, 2]) == ([a, b], [0, 0])
    assert am.segment_sums(pks, [0, 1], [0, 2, 1]) == ([None, None], [1, 1])
    total = None
    for p in pks:
        total = m.g1_add(total, p)
    rest = None
    for p in pks[2:]:
        rest = m.g1_add(rest, p)
    i2, o2 = am.committee_entries([[0, 1]], absent_from=8)
    assert am.segment_sums(pks + [total], i2, o2) == ([rest], [0])
    rows, inf, status = am.sum_rows(pks, idx, off)
    assert rows.shape == (5, 12) and inf.tolist() == [1, 1, 0, 1, 1] and status.tolist() == st
    assert rows[0].tolist() == [0] * 6 + [1] + [0] * 5                  # the identity as the library writes it: (0, 1)


def test_the_timing_tool_parses_its_arguments_and_names_engine_methods_that_exist():
    tool = os.path.join(ROOT, "tools", "time_agg.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--shapes" in out.stdout and "--verify-shapes" in out.stdout and "--table" in out.stdout
    from zkvm_pairings_amd.engine import PairingEngine
    with open(tool) as f:
        text = f.read()
    used = set(re.findall(r"\beng\.([a-z_0-9]+)\(", text))
    assert {"g1_segment_sum", "bls_fast_aggregate_verify", "g1_add", "bls_verify", "hash_to_g2"} <= used
    for name in used:
        assert callable(getattr(PairingEngine, name)), name
