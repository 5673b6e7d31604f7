"""CPU gate of hash-to-G2 and the BLS layer (include/zkp_bls.h): the big-integer model (tests/h2c_model.py) against the RFC 9380 vectors and
against itself - the isogeny, the cofactor, the signs -, the generator's constants, the planning header under sanitizers, and the boundary:
header, ctypes table and Rust block agree, every symbol is exported, no new kernel has a private segment."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import bls12_381_model as m
import h2c_model as h
import outside_groups as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkp_bls.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "bls.rs")
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
NEW = ["zkp_fp_from_wide_be_batch", "zkp_hash_to_field_g2_batch", "zkp_g2_map_from_fields_batch", "zkp_g2_clear_cofactor_batch", "zkp_hash_to_g2_batch",
       "zkp_bls_verify_batch"]
NEW = NEW + [n + "_dev" for n in NEW]


def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "h2c_vectors.json")) as f:
        return json.load(f)


def _seeded_u(count, seed=0x42C):
    g = m.SplitMix64(seed)
    return [(g.below(h.P), g.below(h.P)) for _ in range(count)]


def test_model_gives_the_rfc_vectors():
    v = _vectors()
    assert v["dst"].encode() == h.RFC_DST
    for case in v["vectors"]:
        pt = h.hash_to_g2(case["msg"].encode(), h.RFC_DST)
        assert [hex(pt[0][0]), hex(pt[0][1]), hex(pt[1][0]), hex(pt[1][1])] == [hex(int(x, 16)) for x in case["p"]]


def test_isogeny_lands_on_e2_and_is_a_homomorphism():
    pts = [h.sswu(u)[0] for u in _seeded_u(64)]
    assert all(h.iso_on_curve(p) for p in pts)
    img = [h.iso3(p) for p in pts]
    assert all(m.g2_on_curve(q) for q in img)
    for a, b in zip(pts[:32], pts[32:]):
        assert h.iso3(h.iso_add(a, b)) == m.g2_add(h.iso3(a), h.iso3(b))
    assert h.iso3(h.iso_add(pts[0], pts[0])) == m.g2_add(img[0], img[0])
    # the kernel: both denominators vanish at its abscissa, and a rational point there (there is none when g is no square) has order three
    # and goes to the identity
    assert h._poly(h.ISO_XDEN, h.KERNEL_X) == (0, 0) and h._poly(h.ISO_YDEN, h.KERNEL_X) == (0, 0)
    g = m.f2_add(m.f2_add(m.f2_mul(m.f2_sqr(h.KERNEL_X), h.KERNEL_X), m.f2_mul(h.A_ISO, h.KERNEL_X)), h.B_ISO)
    y = h.f2_sqrt(g)
    if y is not None:
        k = (h.KERNEL_X, y)
        assert h.iso_on_curve(k) and h.iso_add(h.iso_add(k, k), k) is None and h.iso3(k) is None


def test_psi_formula_is_h_eff_and_outputs_have_order_r():
    seeded = [h.iso3(h.sswu(u)[0]) for u in _seeded_u(6, seed=7)]
    fixtures = list(og.g2_points().values())
    on_curve = [q for q in fixtures if m.g2_on_curve(q)]
    assert len(on_curve) >= 2
    for q in seeded + on_curve + [m.G2_GEN]:
        want = h.clear_cofactor_h_eff(q)
        assert h.clear_cofactor_psi(q) == want
        assert want is None or m.g2_mul(want, h.R_ORDER) is None
    assert h.clear_cofactor_psi(None) is None


def test_sswu_signs_the_exceptional_case_and_both_branches():
    us = _seeded_u(24, seed=11)
    branches = set()
    for u in us:
        pt, square = h.sswu(u)
        branches.add(square)
        neg, _ = h.sswu(m.f2_neg(u))
        assert neg == (pt[0], m.f2_neg(pt[1]))
        assert h.sgn0(pt[1]) == h.sgn0(u)
    assert branches == {True, False}
    zero, _ = h.sswu((0, 0))
    assert h.iso_on_curve(zero)
    assert h.map_from_fields(us[0], m.f2_neg(us[0])) is None          # Q + (-Q)
    q = h.iso3(h.sswu(us[0])[0])
    assert h.map_from_fields(us[0], us[0]) == h.clear_cofactor_psi(m.g2_add(q, q))


def test_adversarial_field_elements_have_their_stated_properties():
    """tests/h2c_adversarial.py: what test_gpu_h2c.py feeds the map is what its docstring says, in the model"""
    import h2c_adversarial as ha
    # two facts k_h2c_map leans on: u^2 = -1 / Z has no solution, so Z^2 u^4 + Z u^2 vanishes at u = 0 only; and E' has no point at the
    # isogeny's pole, so no u maps to the identity (which is why there is no such input)
    assert not h.f2_is_square(m.f2_neg(m.f2_inv(h.Z_SSWU)))
    assert not h.f2_is_square(ha.g_iso(h.KERNEL_X))
    pairs = ha.colliding_pairs()
    assert set(pairs) == {"same", "opposite", "cross_same", "cross_opposite"}
    for kind, ps in pairs.items():
        assert len(ps) >= 2, kind
        cross, same = kind.startswith("cross"), kind.endswith("same")
        for u0, u1 in ps:
            assert u1 not in (u0, m.f2_neg(u0))
            (p0, sq0), (p1, sq1) = h.sswu(u0), h.sswu(u1)
            assert sq1 and sq0 == (not cross), kind                       # u1 on the x1 branch; u0 on it unless the pair is a cross pair
            assert ha.x1_of(u1) == p0[0] == p1[0] and (ha.x1_of(u0) == p0[0]) == (not cross)
            q0, q1 = h.iso3(p0), h.iso3(p1)
            assert q0 is not None and q0 == (q1 if same else m.g2_neg(q1)), kind
            for a, b in ((u0, u1), (u1, u0)):
                assert h.map_from_fields(a, b) == (h.clear_cofactor_psi(m.g2_add(q0, q0)) if same else None)
    real = ha.real_g_elements()
    assert set(real) == {"residue", "nonresidue"}
    for kind, us in real.items():
        assert len(us) >= 4 and len(set(us)) == len(us), kind
        for u in us:
            gx = ha.g_iso(ha.x1_of(u))
            (x, y), square = h.sswu(u)
            assert gx[1] == 0 and square and x == ha.x1_of(u)
            assert pow(gx[0], (h.P - 1) // 2, h.P) == (1 if kind == "residue" else h.P - 1)
            assert (y[1] == 0 and y[0]) if kind == "residue" else (y[0] == 0 and y[1])          # a real root / a purely imaginary one
    rows = ha.inputs()
    assert len(rows) == 2 * sum(len(v) for v in pairs.values()) + sum(len(v) for v in real.values()) == len(set(rows)) == 24
    assert {k for k, _, _ in rows} == {a + b for a in pairs for b in ("", "-swapped")} | {a + b for a in real for b in ("", "-second")}
    assert [q is None for q in ha.expected()] == [k.split("-")[0].endswith("opposite") for k, _, _ in rows]
    assert all(q is None or m.g2_torsion_free(q) for q in ha.expected())


# what the inputs of tests/h2c_adversarial.py's cofactor_points reach in k_h2c_clear's additions (sites of h.clear_cofactor_trace)
COFACTOR_BRANCHES = {("A", "p_inf"), ("A", "generic"), ("A", "cancel"), ("C", "p_inf"), ("C", "generic"), ("C", "cancel"),
                     ("B", "p_inf"), ("B", "generic"), ("B", "dbl"),
                     ("F0", "p_inf"), ("F0", "generic"), ("F1", "p_inf"), ("F1", "generic"), ("F2", "p_inf"), ("F2", "generic"),
                     ("F3", "p_inf"), ("F3", "generic"), ("F3", "cancel")}


def test_cofactor_trace_equals_both_formulas_and_reaches_the_stated_branches():
    import h2c_adversarial as ha
    pts, traces = ha.cofactor_points(), ha.cofactor_traces()
    labels = [k for k, _ in pts]
    assert len(set(labels)) == len(pts) == len(traces) and sum(k.startswith("order13*") for k in labels) == 12
    assert {"identity", "generator", "e2-0", "fixture-order13", "fixture-cofactor", "order23", "order262069", "order13+g2", "order262069+g2"} <= set(labels)
    hit = set()
    for (label, q), (got, seen) in zip(pts, traces):
        assert q is None or m.g2_on_curve(q), label
        assert got == h.clear_cofactor_psi(q) == h.clear_cofactor_h_eff(q), label
        hit |= seen
    assert COFACTOR_BRANCHES <= hit, sorted(COFACTOR_BRANCHES - hit)
    # which input takes which: the identity every p_inf of the tail; a point of G2 doubles at B (psi(P) = [x] P = -A); order 13 cancels
    # in both ladders at the prefix 13 = 12 + 1; a point the cofactor kills ends in (-psi^2(2 P)) + psi^2(2 P)
    by = dict(zip(labels, (s for _, s in traces)))
    assert {("B", "p_inf"), ("F0", "p_inf"), ("F3", "p_inf")} <= by["identity"] and ("B", "dbl") in by["generator"]
    assert len(ha.NEAR_ZERO_MULTIPLES) >= 4 and all(("B", "dbl") in by["generator*%d" % k] for k in ha.NEAR_ZERO_MULTIPLES)
    assert all({("A", "cancel"), ("C", "cancel")} <= by["order13*%d" % k] for k in range(1, 13))
    assert all(("F3", "cancel") in by["order%d" % ell] for ell in ha.SMALL_ORDERS[1:])
    # the ladders' other exceptional branches.  #E2 and its prime factors:
    order = 1
    for q, e in ha.E2_FACTORS.items():
        assert all(q % d for d in range(2, 513) if d * d <= q) if q < 1 << 18 else pow(2, q - 1, q) == 1, q      # trial division; Fermat for the two large ones
        order *= q ** e
    assert order == ha.E2_ORDER and m.g2_mul(pts[labels.index("e2-0")][1], order) is None
    # At its additions after the first a ladder holds [v] Q, v in LADDER_ADDS, and adds Q: it doubles iff ord(Q) > 1 divides v - 1, and
    # the operand is at infinity only when the accumulator is as well, which jac_add asks first.  So q_inf is unreachable, and dbl needs a
    # prime factor of #E2 that divides some v - 1: a point of that order is then required to double, and where there is none the branch is
    # absent because no point of E2 reaches it.
    assert h.LADDER_ADDS == tuple(2 * (h.X_ABS >> b) for b in range(63, 0, -1) if (h.X_ABS >> (b - 1)) & 1) and h.X_ABS >> 63 == 1
    doubling = sorted({q for v in h.LADDER_ADDS for q in ha.E2_FACTORS if (v - 1) % q == 0})
    for q in doubling:
        assert ("A", "dbl") in h.clear_cofactor_trace(ha.point_of_order(q))[1], q
    if not doubling:
        assert not {("A", "dbl"), ("C", "dbl"), ("A", "q_inf"), ("C", "q_inf")} & hit
    assert sorted({q for v in h.LADDER_ADDS for q in ha.E2_FACTORS if (v + 1) % q == 0}) == [13]   # the one cancellation: 12 + 1


def test_generator_constants_equal_the_suite():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_constants as gc
    consts, iso = gc.h2c_consts()
    assert iso == (h.ISO_XNUM, h.ISO_XDEN, h.ISO_YNUM, h.ISO_YDEN)
    assert m.f2_mul(m.f2_sqr(h.ISO_XNUM[3]), h.ISO_XNUM[3]) == m.f2_sqr(h.ISO_YNUM[3])
    assert consts["SSWU_A"] == h.A_ISO and consts["SSWU_B"] == h.B_ISO and consts["SSWU_Z"] == h.Z_SSWU
    assert m.f2_mul(consts["SSWU_NBA"], h.A_ISO) == m.f2_neg(h.B_ISO)
    assert consts["ISO_DEN"] == m.f2_neg(h.KERNEL_X)
    # ... and the committed 28-bit header holds them, Montgomery form with R = 2^392, balanced limbs
    hdr = open(os.path.join(CSRC, "zkp_constants28.h")).read()
    r392 = (1 << 392) % h.P
    for name, val in consts.items():
        for c in (0, 1):
            limbs = [int(x) for x in re.search(r"X\(%s_%d, ([-0-9, ]+)\)" % (name, c), hdr).group(1).split(",")]
            assert sum(l << (28 * i) for i, l in enumerate(limbs)) % h.P == val[c] * r392 % h.P, name
    # ... and the 32-bit header (Montgomery form with R = 2^384, twelve limbs), which no kernel reads yet
    hdr = open(os.path.join(CSRC, "zkp_constants.h")).read()
    r384 = (1 << 384) % h.P
    for name, val in consts.items():
        for c in (0, 1):
            limbs = [int(x.rstrip("u"), 16) for x in re.search(r"X\(M_%s_%d, ([0-9a-fx, u]+)\)" % (name, c), hdr).group(1).split(",")]
            assert len(limbs) == 12 and sum(l << (32 * i) for i, l in enumerate(limbs)) == val[c] * r384 % h.P, name


# ----------------------------------------------------------------------------------------------------------------- the planning header


def test_planner_holds_at_the_abi_limits(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "bls_plan_check.cpp"), tmp_path / "bls_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ----------------------------------------------------------------------------------------------------------------- the hash kernels' own text
LENGTHS = (0, 1, 8, 9, 16, 17, 55, 56, 63, 64, 65, 119, 120, 1000)          # both sides of every padding boundary of b_0 (43-byte DST); 72 | 73 below
DST_LENGTHS = (1, 21, 22, 43, 85, 86, 255)                                   # b_i: one block becomes two at 22, two three at 86


@pytest.fixture(scope="module")
def hash_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bls_kernels") / "bls_kernel_host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                         "-Wno-unknown-pragmas", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "bls_kernel_host.cpp")], capture_output=True, text=True,
                        timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _run_hash(exe, tmp_path, dst, msgs, base=0, wide=(), offsets=None):
    """(u rows as bytes, wide reductions as bytes, validation word) of the kernels on host; offsets override the packing of msgs"""
    import struct
    body = b"".join(msgs)
    if offsets is None:
        offsets, at = [base], base
        for x in msgs:
            at += len(x)
            offsets.append(at)
    n = len(offsets) - 1
    data = struct.pack("<4Q", len(dst), n, len(wide), base) + dst + struct.pack("<%dQ" % (n + 1), *offsets) + body[:max(offsets[n], base) - base]
    data += b"".join(v.to_bytes(64, "big") for v in wide)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(data)
    out = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    raw = fout.read_bytes()
    assert len(raw) == 192 * n + 48 * len(wide) + 4
    return raw[:192 * n], raw[192 * n:192 * n + 48 * len(wide)], int.from_bytes(raw[-4:], "little")


def _field_bytes(msgs, dst):
    return b"".join(v.to_bytes(48, "little") for x in msgs for u in h.hash_to_field_g2(x, dst) for v in u)


def _seeded_bytes(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def test_hash_kernels_on_host_equal_the_model_at_every_padding_boundary(hash_exe, tmp_path):
    import random
    rng = random.Random(0x5A)
    msgs = [_seeded_bytes(rng, n) for n in LENGTHS + (72, 73, 2, 3, 31, 33)]
    for dst_len in DST_LENGTHS:
        dst = h.ETH_DST if dst_len == 43 else _seeded_bytes(rng, dst_len)
        use = msgs if dst_len in (43, 255, 1) else msgs[:9]
        u, _, word = _run_hash(hash_exe, tmp_path, dst, use)
        assert word == 0 and u == _field_bytes(use, dst), dst_len
    u, _, _ = _run_hash(hash_exe, tmp_path, h.RFC_DST, [b"", b"abc"])
    assert u == _field_bytes([b"", b"abc"], h.RFC_DST)


@pytest.mark.parametrize("base", [1, 2, 3, (1 << 40) - 1, (1 << 40) + 6])
def test_hash_kernels_on_host_at_unaligned_and_large_offsets(hash_exe, tmp_path, base):
    """the messages start at every alignment, and at offsets near 2^40 through the biased pointer of the host flavour; more than one workgroup"""
    import random
    rng = random.Random(base & 0xFFFF)
    msgs = [_seeded_bytes(rng, n) for n in (37, 4, 5, 6, 7, 0, 64, 13)] + [bytes(range(37))] * (257 if base == 1 else 3)
    u, _, word = _run_hash(hash_exe, tmp_path, h.ETH_DST, msgs, base=base)
    assert word == 0 and u == _field_bytes(msgs, h.ETH_DST)


def test_hash_kernels_on_host_never_follow_decreasing_offsets(hash_exe, tmp_path):
    msgs = [b"first", b"second message", b"third"]
    body = b"".join(msgs)
    off = [0, 5, 2, len(body)]                         # message 1 runs backwards; message 2 is a sound range of the buffer
    u, _, word = _run_hash(hash_exe, tmp_path, h.ETH_DST, msgs, offsets=off)
    assert word == 1 and u == _field_bytes([msgs[0], b"", body[2:]], h.ETH_DST)
    off = [4, 9, 1 << 50, 3]                           # the last offset lies before the first: nothing is sound, nothing is read
    u, _, word = _run_hash(hash_exe, tmp_path, h.ETH_DST, msgs, base=4, offsets=off)
    assert word == 1 and u == _field_bytes([b"", b"", b""], h.ETH_DST)


def test_wide_reduction_on_host_equals_the_integers(hash_exe, tmp_path):
    import random
    q = (1 << 512) // h.P
    vals = [0, 1, h.P - 1, h.P, h.P + 1, (1 << 384) - 1, 1 << 384, (1 << 512) - 1, q * h.P - 1, q * h.P, q * h.P + 1]
    vals += [1 << b for b in range(0, 512, 28)] + [(1 << b) - 1 for b in range(28, 512, 28)]
    vals += [1 << b for b in range(0, 512, 32)] + [(1 << b) - 1 for b in range(32, 512, 32)]
    rng = random.Random(0x51DE)
    vals += [rng.randrange(1 << 512) for _ in range(300)]
    _, red, _ = _run_hash(hash_exe, tmp_path, h.ETH_DST, [], wide=vals)
    assert red == b"".join((v % h.P).to_bytes(48, "little") for v in vals)


def test_the_timing_tool_parses_its_arguments_and_names_engine_methods_that_exist():
    import sys
    tool = os.path.join(ROOT, "tools", "time_bls.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--hash-n" in out.stdout and "--verify-n" in out.stdout
    from zkvm_pairings_amd.engine import PairingEngine
    with open(tool) as f:
        text = f.read()
    used = set(re.findall(r"\beng\.([a-z_0-9]+)\(", text))
    assert {"hash_to_g2", "bls_verify", "compress_points_dev", "decompress_points_dev", "pairing_check_rlc", "pairing_check"} <= used
    for name in used:
        assert callable(getattr(PairingEngine, name)), name


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
    assert sorted(c) == sorted(NEW) == sorted(_lib.BLS_SIGNATURES)
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
    for name, (res, args) in _lib.BLS_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args
    tables = [_lib.SIGNATURES, _lib.POLY_SIGNATURES, _lib.PROVE_SIGNATURES, _lib.FK20_SIGNATURES, _lib.CELLS_SIGNATURES, _lib.RECOVER_SIGNATURES,
              _lib.BLS_SIGNATURES]
    assert sum(len(t) for t in tables) == len(set().union(*tables))
    assert lib.zkp_abi_version() == 4


def test_the_old_boundary_gained_one_module_line():
    names = "|".join(n for n in NEW if not n.endswith("_dev"))
    for other in ("zkp_pairings.h", "zkp_poly.h", "zkp_prove.h", "zkp_fk20.h", "zkp_cells.h", "zkp_recover.h"):
        with open(os.path.join(ROOT, "include", other)) as f:
            assert not re.search(names, f.read()), other
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert len(re.findall(r"^(?:pub )?mod bls;$", lib_rs, re.M)) == 1 and not re.search(names, lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_bls.hip", "zkp_bls_clear.hip", "zkp_bls.hpp", "zkp_bls_plan.hpp", "include/zkp_bls.h"))
    assert os.path.exists(os.path.join(ROOT, "integration", "c", "zkp_bls.c"))
    with open(HEADER) as f:
        text = f.read()
    assert all(x in text for x in ('#include "zkp_pairings.h"', "under ABI version 4", "Slices and workspace", "Cost:", "How", "ZKP_ERR_ARG", "Out of scope"))


def test_every_dev_entry_point_has_a_replay_case_or_a_written_reason():
    import bls_replay_cases as brc
    declared = set(re.findall(r"\b(zkp_\w+_dev)\(", _header_text()))
    table, excluded = brc.table_c_names(), set(brc.EXCLUDED)
    assert declared == {n for n in NEW if n.endswith("_dev")}
    assert not (table & excluded)
    assert declared - (table | excluded) == set(), "no replay case and no reason: %s" % sorted(declared - (table | excluded))
    assert (table | excluded) - declared == set()
    assert all(isinstance(why, str) and len(why) > 20 for why in brc.EXCLUDED.values())
    from zkvm_pairings_amd.engine import PairingEngine
    for c in brc.CASES:
        assert callable(getattr(PairingEngine, c.method)), c.id


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    for name, (_, args) in _lib.BLS_SIGNATURES.items():
        assert getattr(lib, name)(*[None if a is ctypes.c_void_p else 0 for a in args]) == -1, name
    for name in ("hash_to_g2", "hash_to_field_g2", "g2_map_from_fields", "g2_clear_cofactor", "fp_from_wide_be", "bls_verify"):
        assert callable(getattr(z.PairingEngine, name))
    for name in ("hash_to_g2", "bls_sign_batch", "bls_verify_batch", "bls_verify_each", "bls_verify_batch_compressed", "bls_verify_each_compressed"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.synthetic.bls_instance)


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_are_there_and_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_h2" in n or "k_bls_" in n}
    for part in ("k_h2c_tails", "k_h2fE", "k_h2c_wide", "k_h2c_map", "k_h2c_clearILb0", "k_h2c_clearILb1", "k_bls_init", "k_bls_fold", "k_bls_finish"):
        assert sum(part in n for n in new) == 1, part
    assert len(new) == 9, sorted(new)
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)
    counted = ("k_ntt_pass", "k_msm_", "k_add28", "k_g1_mul_endo28", "k_fr_", "k_kzg_", "k_prove_", "k_spmv", "k_poly_coset", "k_open_quot", "k_rlc_",
               "k_g16_", "k_frinv_", "k_freval_", "k_zero_fill", "k_coop", "k_g1ntt_", "k_fk20_", "k_cell_", "k_rec_")
    assert not [n for n in new for x in counted if x in n]
    # the codec whose helpers moved into the shared header kept its registers
    for n, v in k.items():
        if "k_g2_decompress" in n:
            assert v["vgpr"] <= 274 and v["spill"] == 0 and v["scratch"] == 0, (n, v)
