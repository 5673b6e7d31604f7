"""CPU gate of hash-to-G1 and the min-sig BLS layer (no GPU): the big-integer model against the RFC's vectors, the generator's derived
isogeny against the model's pointwise one and the committed constant headers, the kernels of zkp_bls_minsig.hip compiled for the host under
sanitizers against the model, the planning header under sanitizers, and the boundary: header, ctypes and Rust signatures."""
import ctypes
import json
import os
import random
import re
import struct
import subprocess
import sys

import pytest

import h2g1_adversarial as ha
import h2g1_model as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "zkp_bls_minsig.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "bls_minsig.rs")
P = g.P
m = g.m
NEW = ["zkp_hash_to_field_g1_batch", "zkp_g1_map_from_fields_batch", "zkp_g1_clear_cofactor_batch", "zkp_hash_to_g1_batch", "zkp_bls_minsig_verify_batch",
       "zkp_bls_minsig_verify_samekey_batch"]
NEW = NEW + [n + "_dev" for n in NEW]
LENGTHS = (0, 1, 8, 9, 16, 17, 55, 56, 63, 64, 65, 119, 120, 1000)          # tests/test_h2c_cpu.py's: both sides of every padding boundary of b_0
DST_LENGTHS = (1, 21, 22, 43, 85, 86, 255)


def _kat():
    with open(os.path.join(ROOT, "tests", "golden", "h2c_g1_vectors.json")) as f:
        return json.load(f)


# ----------------------------------------------------------------------------------------------------------------- the model, the constants
def test_model_gives_the_rfc_vectors_and_only_the_scaling_11_does():
    kat = _kat()
    dst = kat["dst"].encode()
    assert dst == g.RFC_DST and len(kat["vectors"]) == 5
    assert list(g.hash_to_field_g1(b"", dst)) == [int(x, 16) for x in kat["u_empty"]]
    for v in kat["vectors"]:
        pt = g.hash_to_g1(v["msg"].encode(), dst)
        assert pt == tuple(int(c, 16) for c in v["p"]) and g.in_g1(pt), v["msg"]
    first = tuple(int(c, 16) for c in kat["vectors"][0]["p"])
    assert [s for s in g.scalings() if g.hash_to_g1(b"", dst, s) == first] == [11]


def test_the_kernel_the_image_curve_and_the_homomorphism():
    pts = g.kernel_points()
    assert all(g.iso_on_curve(q) and g.ec_mul(q, 11, g.A_ISO) is None for q in pts) and len({q[0] for q in pts}) == 5
    rng = random.Random(3)
    some = []
    while len(some) < 3:
        x = rng.randrange(P)
        y = m.fp_sqrt(g.g_iso(x))
        if y is not None:
            some.append((x, y))
    for q in some:
        assert g.ec_mul(q, g.N_E, g.A_ISO) is None                                      # E1' is isogenous to E
        v = g.velu(q)
        assert v[1] * v[1] % P == (v[0] ** 3 + 4 * 11 ** 6) % P                        # Velu lands on y^2 = x^3 + 4 * 11^6
        assert g.e_on_curve(g.iso11(q))
    a, b = some[0], some[1]
    assert g.iso11(g.ec_add(a, b, g.A_ISO)) == g.e_add(g.iso11(a), g.iso11(b))
    assert g.iso11(pts[2]) is None and g.iso11(g.ec_add(a, pts[0], g.A_ISO)) == g.iso11(a)
    assert g.e_mul((0, 2), 3) is None and g.clear_cofactor((0, 2)) is None and g.in_g1(g.clear_cofactor(g.iso11(b)))


def test_adversarial_inputs_have_their_stated_properties():
    z = g.Z_SSWU
    for u in ha.exceptional_u():
        assert (z * z * pow(u, 4, P) + z * u * u) % P == 0
    poles = ha.pole_u()
    assert len(poles) == 16 and sum(sq for _, sq in poles) == 8 and {(P - u) for u, _ in poles} == {u for u, _ in poles}
    u = poles[0][0]
    assert g.sswu(P - u)[0] == g.ec_neg(g.sswu(u)[0])                                   # u and -u map to opposite points
    names = [c[0] for c in ha.field_cases()]
    assert len(set(names)) == len(names) and {"doubling", "cancel", "square", "nonsquare", "p_minus_1"} <= set(names)
    assert {c[0] for c in ha.point_cases()} >= {"order3_plus", "order3_minus", "order11", "identity", "g1_random", "order3_plus_g1", "outside0"}


def test_generator_isogeny_equals_the_model_and_the_headers_hold_it():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_constants as gc
    consts, iso = gc.g1h_consts()
    xn, xd, yn, yd = iso
    assert [len(c) for c in iso] == [12, 11, 16, 16] and xd[-1] == 1 and yd[-1] == 1
    rng = random.Random(5)
    n = 0
    while n < 4:
        x = rng.randrange(P)
        y = m.fp_sqrt(g.g_iso(x))
        if y is None:
            continue
        n += 1
        want = g.iso11((x, y))
        got = (gc._qeval(xn, x) * m.fp_inv(gc._qeval(xd, x)) % P, y * gc._qeval(yn, x) % P * m.fp_inv(gc._qeval(yd, x)) % P)
        assert got == want
    for q in g.kernel_points():
        assert gc._qeval(xd, q[0]) == 0 and gc._qeval(yd, q[0]) == 0                   # the poles
    assert consts["G1SSWU_A"] == g.A_ISO and consts["G1SSWU_B"] == g.B_ISO and consts["G1SSWU_Z"] == g.Z_SSWU
    assert consts["G1SSWU_C2"] ** 2 % P == P - g.Z_SSWU and len(consts) == 4 + 55
    hdr = open(os.path.join(CSRC, "zkp_constants28.h")).read()
    r392 = (1 << 392) % P
    order = re.findall(r"X\((G1[A-Z0-9_]+),", hdr.split("ZKP28_G1H_CONST_LIST")[1])
    assert order == list(consts)                                                        # the kernels index the list by position
    for name, val in consts.items():
        limbs = [int(x) for x in re.search(r"X\(%s, ([-0-9, ]+)\)" % name, hdr).group(1).split(",")]
        assert len(limbs) == 14 and sum(l << (28 * i) for i, l in enumerate(limbs)) % P == val * r392 % P, name
    hdr = open(os.path.join(CSRC, "zkp_constants.h")).read()
    r384 = (1 << 384) % P
    for name, val in consts.items():
        limbs = [int(x.rstrip("u"), 16) for x in re.search(r"X\(M_%s, ([0-9a-fx, u]+)\)" % name, hdr).group(1).split(",")]
        assert len(limbs) == 12 and sum(l << (32 * i) for i, l in enumerate(limbs)) == val * r384 % P, name


# ----------------------------------------------------------------------------------------------------------------- the planning header
def test_planner_holds_at_the_abi_limits(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "minsig_plan_check.cpp"), tmp_path / "minsig_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ----------------------------------------------------------------------------------------------------------------- the kernels' own text
@pytest.fixture(scope="module")
def kernel_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("minsig_kernels") / "minsig_kernel_host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                         "-Wno-unknown-pragmas", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "minsig_kernel_host.cpp")], capture_output=True, text=True,
                        timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _run(exe, tmp_path, dst, msgs, base=0, offsets=None, fields=(), points=()):
    """(u rows as bytes, projective points of the map, projective points of the cofactor, validation word) of the kernels on host"""
    body = b"".join(msgs)
    if offsets is None:
        offsets, at = [base], base
        for x in msgs:
            at += len(x)
            offsets.append(at)
    n = len(offsets) - 1
    data = struct.pack("<5Q", len(dst), n, len(fields), len(points), base) + dst + struct.pack("<%dQ" % (n + 1), *offsets) + body[:max(offsets[n], base) - base]
    data += b"".join(u.to_bytes(48, "little") for pair in fields for u in pair)
    data += b"".join(int(w).to_bytes(8, "little") for pt in points for w in g.g1_words(pt)[0]) + bytes(1 if pt is None else 0 for pt in points)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(data)
    out = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    raw = fout.read_bytes()
    assert len(raw) == 96 * n + 144 * (len(fields) + len(points)) + 4

    def proj(b):
        x, y, z = [int.from_bytes(b[48 * i:48 * i + 48], "little") for i in range(3)]
        if z == 0:
            assert x == 0 and y != 0                                                    # the identity is (0 : y : 0)
            return None
        zi = m.fp_inv(z)
        return (x * zi % P, y * zi % P)
    at = 96 * n
    mapped = [proj(raw[at + 144 * i:at + 144 * (i + 1)]) for i in range(len(fields))]
    at += 144 * len(fields)
    cleared = [proj(raw[at + 144 * i:at + 144 * (i + 1)]) for i in range(len(points))]
    return raw[:96 * n], mapped, cleared, int.from_bytes(raw[-4:], "little")


def _field_bytes(msgs, dst):
    return b"".join(v.to_bytes(48, "little") for x in msgs for v in g.hash_to_field_g1(x, dst))


def _seeded_bytes(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def test_hash_kernel_on_host_equals_the_model_at_every_padding_boundary(kernel_exe, tmp_path):
    rng = random.Random(0x5B)
    msgs = [_seeded_bytes(rng, n) for n in LENGTHS + (72, 73, 2, 3, 31, 33)]
    for dst_len in DST_LENGTHS:
        dst = g.QUICKNET_DST if dst_len == 43 else _seeded_bytes(rng, dst_len)
        use = msgs if dst_len in (43, 255, 1) else msgs[:9]
        u, _, _, word = _run(kernel_exe, tmp_path, dst, use)
        assert word == 0 and u == _field_bytes(use, dst), dst_len
    u, _, _, _ = _run(kernel_exe, tmp_path, g.RFC_DST, [b"", b"abc"])
    assert u == _field_bytes([b"", b"abc"], g.RFC_DST)


@pytest.mark.parametrize("base", [1, 2, 3, (1 << 40) - 1, (1 << 40) + 6])
def test_hash_kernel_on_host_at_unaligned_and_large_offsets(kernel_exe, tmp_path, base):
    rng = random.Random(base & 0xFFFF)
    msgs = [_seeded_bytes(rng, n) for n in (37, 4, 5, 6, 7, 0, 64, 13)] + [bytes(range(37))] * (257 if base == 1 else 3)
    u, _, _, word = _run(kernel_exe, tmp_path, g.QUICKNET_DST, msgs, base=base)
    assert word == 0 and u == _field_bytes(msgs, g.QUICKNET_DST)


def test_hash_kernel_on_host_never_follows_decreasing_offsets(kernel_exe, tmp_path):
    msgs = [b"first", b"second message", b"third"]
    body = b"".join(msgs)
    u, _, _, word = _run(kernel_exe, tmp_path, g.QUICKNET_DST, msgs, offsets=[0, 5, 2, len(body)])
    assert word == 1 and u == _field_bytes([msgs[0], b"", body[2:]], g.QUICKNET_DST)
    u, _, _, word = _run(kernel_exe, tmp_path, g.QUICKNET_DST, msgs, base=4, offsets=[4, 9, 1 << 50, 3])
    assert word == 1 and u == _field_bytes([b"", b"", b""], g.QUICKNET_DST)


def test_map_and_cofactor_kernels_on_host_equal_the_model_on_adversarial_inputs(kernel_exe, tmp_path):
    """ZKP_FP28_HOST covers everything k_g1h_map and k_g1h_clear use: the exceptional u, the sixteen poles, a doubling, a cancellation,
    points of order 3 and 11, the identity, points in and outside G1 - bit-exact values without a GPU (65 u pairs: two wavefronts)"""
    rng = random.Random(0x5C)
    fields = [(c[1], c[2]) for c in ha.field_cases()] + [(rng.randrange(P), rng.randrange(P)) for _ in range(18)]
    points = [c[1] for c in ha.point_cases()]
    assert len(fields) == 65
    _, mapped, cleared, _ = _run(kernel_exe, tmp_path, g.RFC_DST, [], fields=fields, points=points)
    for (u0, u1), got, case in zip(fields, mapped, [c[0] for c in ha.field_cases()] + ["random"] * 18):
        assert got == g.map_from_fields(u0, u1), case
    for pt, got, case in zip(points, cleared, ha.point_cases()):
        assert got == g.clear_cofactor(pt) and g.in_g1(got), case[0]


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
        assert re.search(r"\b(int|unsigned|uint32_t|int32_t)\b", t), t
        return "int"
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
    return {name: (kind(ret), [kind(p.split(":", 1)[1]) for p in _split_params(params)])
            for name, params, ret in re.findall(r"pub fn (zkp_[a-z0-9_]+)\s*\(([^)]*)\)\s*->\s*([^;]+);", text)}


def test_header_ctypes_and_rust_agree_and_every_symbol_is_exported():
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    c, rust = _c_signatures(), _rust_signatures()
    assert sorted(c) == sorted(NEW) == sorted(_lib.BLS_MINSIG_SIGNATURES) == sorted(rust)
    for name, sig in c.items():
        assert hasattr(lib, name), "libzkp_pairings.so does not export %s" % name
        assert rust[name] == sig, (name, "rust", rust[name], "header", sig)
        if name.endswith("_dev"):
            assert sig[1][-1] == "ptr" and c[name[:-4]] == (sig[0], sig[1][:-1]), name

    def ckind(t):
        if t is ctypes.c_size_t:
            return "size"
        if t in (ctypes.c_int, ctypes.c_uint, ctypes.c_uint32):
            return "int"
        assert t is ctypes.c_void_p, t
        return "ptr"
    for name, (res, args) in _lib.BLS_MINSIG_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args
    tables = [_lib.SIGNATURES, _lib.POLY_SIGNATURES, _lib.PROVE_SIGNATURES, _lib.FK20_SIGNATURES, _lib.CELLS_SIGNATURES, _lib.RECOVER_SIGNATURES,
              _lib.BLS_SIGNATURES, _lib.AGG_SIGNATURES, _lib.GRP_SIGNATURES, _lib.BLS_MINSIG_SIGNATURES]
    assert sum(len(t) for t in tables) == len(set().union(*tables))                     # the tables are disjoint
    assert lib.zkp_abi_version() == 4


def test_the_old_boundary_gained_one_module_line_and_the_new_header_its_sections():
    names = "|".join(n for n in NEW if not n.endswith("_dev"))
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "zkp_bls_minsig.h":
            with open(os.path.join(ROOT, "include", other)) as f:
                assert not re.search(names, f.read()), other
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert len(re.findall(r"^(?:pub )?mod bls_minsig;$", lib_rs, re.M)) == 1 and not re.search(names, lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_bls_minsig.hip", "zkp_bls_minsig.hpp", "zkp_bls_minsig_plan.hpp", "zkp_h2f.hpp", "include/zkp_bls_minsig.h"))
    assert os.path.exists(os.path.join(ROOT, "integration", "c", "zkp_bls_minsig.c"))
    with open(HEADER) as f:
        text = f.read()
    assert all(x in text for x in ('#include "zkp_bls.h"', "under ABI version 4", "Slices and workspace", "Cost:", "How", "ZKP_ERR_ARG", "Out of scope"))


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    for name, (_, args) in _lib.BLS_MINSIG_SIGNATURES.items():
        assert getattr(lib, name)(*[None if a is ctypes.c_void_p else 0 for a in args]) == -1, name
    for name in ("hash_to_field_g1", "g1_map_from_fields", "g1_clear_cofactor", "hash_to_g1", "bls_minsig_verify", "bls_minsig_verify_samekey"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("hash_to_g1", "bls_minsig_keygen_batch", "bls_minsig_sign_batch", "bls_minsig_verify_batch", "bls_minsig_verify_samekey_batch",
                 "bls_minsig_verify_each", "bls_minsig_verify_batch_compressed", "bls_minsig_verify_each_compressed"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.synthetic.bls_minsig_instance)


def test_new_kernels_are_there_and_do_not_spill():
    """no skip: the package does not import without the built library, and the facts DESIGN 3.14 quotes are read from it"""
    from test_codeobject import READELF, SO, _kernels
    assert os.path.exists(SO) and os.path.exists(READELF), (SO, READELF)
    new = {n: v for n, v in _kernels().items() if "k_g1h_" in n}
    for part in ("k_g1h_tails", "k_g1h_field", "k_g1h_map", "k_g1h_clearILb0", "k_g1h_clearILb1", "k_g1h_affine", "k_g1h_init", "k_g1h_rows", "k_g1h_fold",
                 "k_g1h_finish"):
        assert sum(part in n for n in new) == 1, part
    assert len(new) == 10, sorted(new)
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["lds"] == (8192 if "affine" in n else 0), (n, v)


def test_every_dev_entry_point_has_a_replay_case_or_a_written_reason():
    import minsig_replay_cases as mrc
    declared = set(re.findall(r"\b(zkp_\w+_dev)\(", _header_text()))
    table, excluded = mrc.table_c_names(), set(mrc.EXCLUDED)
    assert declared == {n for n in NEW if n.endswith("_dev")}
    assert not (table & excluded)
    assert declared - (table | excluded) == set(), "no replay case and no reason: %s" % sorted(declared - (table | excluded))
    assert (table | excluded) - declared == set()
    assert all(isinstance(why, str) and len(why) > 20 for why in mrc.EXCLUDED.values())
    from zkvm_pairings_amd.engine import PairingEngine
    for c in mrc.CASES:
        assert callable(getattr(PairingEngine, c.method)), c.id
    # the sets of a case have one shape, and the verifiers' middle set is the one that must fail
    for c in mrc.CASES[:1] + mrc.CASES[-2:]:
        sets, want = c.make(None, c.shape, 1)
        assert len(sets) == 3 and all({k: v.shape for k, v in s.items()} == {k: v.shape for k, v in sets[0].items()} for s in sets)
        if "verify" in c.id:
            assert [int(w[0][0]) for w in want] == [1, 0, 1]


def test_the_timing_tool_parses_its_arguments_and_names_engine_methods_that_exist():
    tool = os.path.join(ROOT, "tools", "time_minsig.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--reps" in out.stdout and "--n" in out.stdout and "--out" in out.stdout
    from zkvm_pairings_amd.engine import PairingEngine
    with open(tool) as f:
        text = f.read()
    assert '"1024,16384,262144"' in text and "default=5" in text                       # 2^10, 2^14, 2^18; medians of 5
    used = set(re.findall(r"\beng\.([a-z_0-9]+)\(", text))
    assert {"hash_to_g1", "hash_to_g2", "hash_to_field_g1", "bls_minsig_verify", "bls_verify", "bls_minsig_verify_samekey"} <= used
    for name in used:
        assert callable(getattr(PairingEngine, name)), name
