"""CPU gate of the layer that verifies BLS signatures grouped by message (include/zkp_bls_grouped.h): the bilinearity the feature stands
on, on the big-integer model; the planning header under sanitizers at the ABI maxima and around every power of the run length; the index
kernels compiled for the host and run as written on exactly allocated buffers against the model (tests/grp_model.py); the boundary -
header, ctypes table and Rust block agree, every symbol is exported and refuses a null context, every _dev entry has a replay case -; the
code object's k_grp_* set; the Python helpers against the model; the timing tool."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import agg_model as am
import grp_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkp_bls_grouped.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "bls_grouped.rs")
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
NEW = ["zkp_g1_scaled_segment_sum_batch", "zkp_bls_verify_grouped_batch", "zkp_bls_fast_aggregate_verify_grouped_batch"]
NEW = NEW + [n + "_dev" for n in NEW]
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror"]


# ----------------------------------------------------------------------------------------------------------------- the model
def test_the_grouped_product_equals_the_ungrouped_product_on_the_model():
    """n = 6 signatures over m = 3 messages, messages out of order: prod_i e([r_i] pk_i, H(m_i)) and prod_g e(sum [r_i] pk_i, H(m_g)) are
    the same element of Gt - also for a forged batch, where neither is one"""
    import zkvm_pairings_amd as z
    sks, pks = am.key_table(gm.N_TABLE)
    msgs = [am.MESSAGES[g] for g in (1, 0, 1, 2, 0, 1)]
    signers = [3, 9, 27, 41, 5, 60]
    sigs = [am.sign(x, sks[r]) for x, r in zip(msgs, signers)]
    rand = gm.rand_pairs(gm.rand_rows(6, 11))
    perm, distinct, grp_off = gm.group_by_message(msgs)
    assert (perm, distinct, grp_off) == ([0, 2, 5, 1, 4, 3], [am.MESSAGES[1], am.MESSAGES[0], am.MESSAGES[2]], [0, 3, 5, 6])
    got = z.group_by_message(msgs)
    assert (got[0].tolist(), got[1], got[2].tolist()) == (perm, distinct, grp_off) and got[0].dtype == np.int64 and got[2].dtype == np.uint64
    take = lambda xs: [xs[i] for i in perm]
    for forged in (False, True):
        ss = list(sigs)
        if forged:
            ss[0], ss[2] = ss[2], ss[0]                  # two signatures of one message swapped: their sum is unchanged
        flat = gm.m.final_exponentiation(gm.product_ungrouped([pks[r] for r in signers], msgs, ss, rand))
        grouped = gm.m.final_exponentiation(gm.product_grouped(take([pks[r] for r in signers]), distinct, grp_off, take(ss), take(rand)))
        assert flat == grouped and (flat == gm.m.f12_one()) is not forged


def test_group_by_message_on_the_edges():
    import zkvm_pairings_amd as z
    perm, distinct, grp_off = z.group_by_message([])
    assert perm.size == 0 and distinct == [] and grp_off.tolist() == [0]
    perm, distinct, grp_off = z.group_by_message([b"", bytearray(b"x"), b"", b"x"])
    assert (perm.tolist(), distinct, grp_off.tolist()) == gm.group_by_message([b"", b"x", b"", b"x"]) == ([0, 2, 1, 3], [b"", b"x"], [0, 2, 4])


# ----------------------------------------------------------------------------------------------------------------- the planning header
def test_planner_holds_at_the_abi_limits_and_around_every_power_of_the_run(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "grp_plan_check.cpp"), tmp_path / "grp_plan_check"
    subprocess.check_call(SAN + ["-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ----------------------------------------------------------------------------------------------------------------- the index kernels' own text
@pytest.fixture(scope="module")
def index_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grp_kernels") / "grp_kernel_host")
    cc = subprocess.run(SAN + ["-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "grp_kernel_host.cpp")], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _run_index(exe, tmp_path, n, seg_off):
    """(keys, status, the call's word, the validation word) of k_grp_check and k_grp_keys on host"""
    n_seg = len(seg_off) - 1
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<2Q", n, n_seg) + struct.pack("<%dQ" % (n_seg + 1), *seg_off))
    out = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    raw = fout.read_bytes()
    assert len(raw) == 4 * n + n_seg + 8
    return list(struct.unpack_from("<%dI" % n, raw, 0)), list(raw[4 * n:4 * n + n_seg]), int.from_bytes(raw[-8:-4], "little"), int.from_bytes(raw[-4:], "little")


def _offsets(lens):
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    return off


WELL_FORMED = [(0, 0, 3, 0, 0, 1, 2, 0), (5,), (0,), (0, 0), (1, 31, 1, 32, 33, 0, 64, 0, 0, 2), (1,) * 300, (700, 0, 1)]


@pytest.mark.parametrize("lens", WELL_FORMED, ids=[str(i) for i in range(len(WELL_FORMED))])
def test_index_kernels_on_host_equal_the_model_on_well_formed_offsets(index_exe, tmp_path, lens):
    """empty groups first, last and next to each other; more than one workgroup of signatures and of offsets"""
    off = _offsets(lens)
    keys, status, word, bad = _run_index(index_exe, tmp_path, off[-1], off)
    assert (keys, word) == gm.keys(off[-1], off) and status == [0] * len(lens) and (word, bad) == (0, 0)
    assert all(k & gm.KEY_FLAG for k in keys) and all(off[k & 0x7FFFFFFF] <= i < off[(k & 0x7FFFFFFF) + 1] for i, k in enumerate(keys))


MALFORMED = {"decreasing": [0, 4, 3, 7, 7], "first-not-zero": [1, 4, 5, 7, 7], "last-beyond": [0, 4, 5, 7, 8], "last-below": [0, 4, 5, 6, 6],
             "decreasing-far": [0, 1 << 50, 3, 7, 7], "near-2^63": [0, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, 7], "all-huge": [1 << 60, 1 << 61, 1 << 62, 1 << 63, 7]}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_index_kernels_on_host_follow_no_malformed_offset(index_exe, tmp_path, kind):
    """every key is KEY_NONE, both words are set, and (the buffers are exact) nothing outside seg_off, keys and status is touched"""
    off = MALFORMED[kind]
    keys, status, word, bad = _run_index(index_exe, tmp_path, 7, off)
    assert (keys, word) == gm.keys(7, off) and keys == [gm.KEY_NONE] * 7 and (word, bad) == (1, 1)
    assert status == [0] * 4                             # k_grp_affine turns the word into every status


def test_index_kernels_on_host_with_no_group_and_with_no_signature(index_exe, tmp_path):
    assert _run_index(index_exe, tmp_path, 0, [0]) == ([], [], 0, 0)
    assert _run_index(index_exe, tmp_path, 0, [0, 0, 0]) == ([], [0, 0], 0, 0)
    keys, _, word, bad = _run_index(index_exe, tmp_path, 2, [0])                      # signatures and no group to hold them
    assert keys == [gm.KEY_NONE] * 2 and (word, bad) == (1, 1)


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
    assert sorted(c) == sorted(NEW) == sorted(_lib.GRP_SIGNATURES)
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
    for name, (res, args) in _lib.GRP_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args
    tables = [_lib.SIGNATURES, _lib.POLY_SIGNATURES, _lib.PROVE_SIGNATURES, _lib.FK20_SIGNATURES, _lib.CELLS_SIGNATURES, _lib.RECOVER_SIGNATURES,
              _lib.BLS_SIGNATURES, _lib.AGG_SIGNATURES, _lib.GRP_SIGNATURES]
    assert sum(len(t) for t in tables) == len(set().union(*tables))
    assert lib.zkp_abi_version() == 4


def test_the_old_boundary_gained_one_module_line():
    names = "|".join(n for n in NEW if not n.endswith("_dev"))
    for other in ("zkp_pairings.h", "zkp_poly.h", "zkp_prove.h", "zkp_fk20.h", "zkp_cells.h", "zkp_recover.h", "zkp_bls.h", "zkp_bls_agg.h"):
        with open(os.path.join(ROOT, "include", other)) as f:
            assert not re.search(names, f.read()), other
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert len(re.findall(r"^(?:pub )?mod bls_grouped;$", lib_rs, re.M)) == 1 and not re.search(names, lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_bls_grouped.hip", "zkp_bls_grouped.hpp", "zkp_bls_grouped_plan.hpp", "include/zkp_bls_grouped.h"))
    assert os.path.exists(os.path.join(ROOT, "integration", "c", "zkp_bls_grouped.c"))
    with open(HEADER) as f:
        text = f.read()
    assert all(x in text for x in ('#include "zkp_bls_agg.h"', "under ABI version 4", "Slices and workspace", "Cost:", "How", "ZKP_ERR_ARG", "Out of scope"))
    # the out-of-scope line of the eighth header keeps its wording; the ninth says where the follow-up went
    with open(os.path.join(ROOT, "include", "zkp_bls_agg.h")) as f:
        assert "the\n * follow-up, on this segment sum)" in f.read()
    assert "follow-up" in text and "zkp_bls_agg.h" in text
    # the driver: the accumulation is the MSM's on Jacobian records, one pairing path, one scaling
    with open(os.path.join(CSRC, "zkp_bls_grouped.hip")) as f:
        unit = f.read()
    assert "msm_accum(1, /*level0=*/false" in unit and "grp_scale(" in unit and "hipMemsetAsync" not in unit and "hipMalloc" not in unit
    assert "rlc_check_dev" not in unit and "coop_g1_mul_endo" not in unit and unit.count("ctxop::miller_product(") == 2 and unit.count("ctxop::gt_is_one(") == 1
    with open(os.path.join(CSRC, "zkp_coop.hip")) as f:
        coop = f.read()
    assert coop.count("k_grp_scale(") == 1 and "jrec_st<1>(rec, i, 0, p);" in coop


def test_every_dev_entry_point_has_a_replay_case_or_a_written_reason():
    import grp_replay_cases as grc
    declared = set(re.findall(r"\b(zkp_\w+_dev)\(", _header_text()))
    table, excluded = grc.table_c_names(), set(grc.EXCLUDED)
    assert declared == {n for n in NEW if n.endswith("_dev")}
    assert not (table & excluded)
    assert declared - (table | excluded) == set(), "no replay case and no reason: %s" % sorted(declared - (table | excluded))
    assert (table | excluded) - declared == set()
    assert all(isinstance(why, str) and len(why) > 20 for why in grc.EXCLUDED.values())
    from zkvm_pairings_amd.engine import PairingEngine
    for c in grc.CASES:
        assert callable(getattr(PairingEngine, c.method)), c.id
        assert c.shape[1] > 32 >= c.small[1], c.id                   # two accumulation levels under capture, one in the smaller call


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    for name, (_, args) in _lib.GRP_SIGNATURES.items():
        assert getattr(lib, name)(*[None if a is ctypes.c_void_p else 0 for a in args]) == -1, name
    for name in ("g1_scaled_segment_sum", "bls_verify_grouped", "bls_fast_aggregate_verify_grouped"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("group_by_message", "bls_verify_grouped_batch", "bls_fast_aggregate_verify_grouped_batch"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.synthetic.bls_grouped_instance)


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_are_there_and_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_grp_" in n}
    parts = ("k_grp_zero", "k_grp_check", "k_grp_keys", "k_grp_scale", "k_grp_affine", "k_grp_init", "k_grp_fold", "k_grp_scalars", "k_grp_committees",
             "k_grp_finish", "k_grp_set")
    for part in parts:
        assert sum(part in n for n in new) == 1, part
    assert len(new) == len(parts), sorted(new)
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)
    scale = [v for n, v in new.items() if "k_grp_scale" in n][0]
    assert scale["lds"] == 20480 and scale["vgpr"] <= 256             # P and T in five LDS slots: two workgroups per SIMD, as the launch bounds ask
    assert [v["lds"] for n, v in new.items() if "k_grp_affine" in n] == [8192]          # two planes of 64 values: prefix and suffix products
    counted = ("k_ntt_pass", "k_msm_", "k_add28", "k_g1_mul_endo28", "k_fr_", "k_kzg_", "k_prove_", "k_spmv", "k_poly_coset", "k_open_quot", "k_rlc_",
               "k_g16_", "k_frinv_", "k_freval_", "k_zero_fill", "k_coop", "k_g1ntt_", "k_fk20_", "k_cell_", "k_rec_", "k_h2", "k_bls_", "k_agg_")
    assert not [n for n in new for x in counted if x in n]


def test_the_timing_tool_parses_its_arguments_and_names_engine_methods_that_exist():
    tool = os.path.join(ROOT, "tools", "time_grouped.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--n" in out.stdout and "--messages" in out.stdout and "--committee" in out.stdout
    from zkvm_pairings_amd.engine import PairingEngine
    with open(tool) as f:
        text = f.read()
    used = set(re.findall(r"\beng\.([a-z_0-9]+)\(", text))
    assert {"bls_verify_grouped", "bls_verify", "bls_fast_aggregate_verify_grouped", "bls_fast_aggregate_verify", "g1_scaled_segment_sum", "g1_mul_endo",
            "g1_segment_sum"} <= used
    for name in used:
        assert callable(getattr(PairingEngine, name)), name
