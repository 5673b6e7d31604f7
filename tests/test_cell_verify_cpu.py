"""CPU gate for the tests of zkp_kzg_cell_verify_batch (tests/test_gpu_cell_verify.py): the forged batches of tests/cell_verify_cases.py on
the model - each holds in the combined equation (cells_model.batch_holds) under its crafted scalars and under no others -, the degenerate
batches, and the GPU tests' shapes held to the planners' own arithmetic by a small g++ program under ASan and UBSan
(tests/cell_verify_plan_check.cpp, a child process): the parts and tiles of the fold, the passes and the workspace of the inverse
transform, the verifier's layout under every flag combination."""
import os
import random
import re
import subprocess

import pytest

import cell_verify_cases as cv
import cells_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
R = cv.R
MODEL_SHAPES = [(4, 2, 1, True), (4, 2, 1, False), (4, 0, 1, True), (3, 3, 0, True)]


def other_scalars(b, i, j, seed):
    """(what, batch): only b_j changed by one bit, only a_i changed by one bit, fresh scalars"""
    return [("b_j ^ 1", b.with_pair(j, b=b.rand[j][1] ^ 1)), ("a_i ^ 2", b.with_pair(i, a=b.rand[i][0] ^ 2)),
            ("fresh", b.with_rand(cv.pairs(random.Random(seed), b.n)))]


@pytest.mark.parametrize("shape", MODEL_SHAPES, ids=["N16-l4-bitrev", "N16-l4-natural", "N16-l1", "N8-l8-M1"])
def test_every_forgery_holds_under_its_crafted_scalars_and_under_no_others(shape):
    n, l = 7, 1 << shape[1]
    base = cv.valid_batch(shape, n, 0xF0 + sum(shape))
    assert cv.want(base) and all(cv.want_each(base))
    rng = random.Random(0xF1 + sum(shape))
    for i, j in ((0, n - 1), (n // 2, 1)):
        for name, forged, half in cv.forgeries(base, i, j, sorted({0, 1 % l, l - 1}), rng):
            what = (shape, name, i, j)
            assert cv.holds(forged) and cv.want(forged), what
            assert not cv.holds(half), what
            for how, other in other_scalars(forged, i, j, 0xF2 + i):
                assert not cv.holds(other), (what, how)
            # both cells are false on their own: the per-cell path names them
            each = cv.want_each(forged)
            assert not each[i] and not each[j] and sum(each) == n - 2, what
        d = rng.randrange(1, R)
        plain = cv.shift_commitments(base, i, j, d)
        assert not cv.holds(plain) and not cv.holds(cv.shift_commitments(base, i, j, d, half=True))
        assert cv.holds(plain.with_pair(j, *plain.rand[i]))                            # equal scalars cannot tell: why they are random


def test_the_scalar_of_the_model_is_the_one_the_rlc_tests_pin():
    assert cv.Z2 == 0xAC45A4010001A402_0000000100000000
    assert cv.scalar((3, 5)) == 3 + 5 * cv.Z2 and cv.scalar((2 ** 64 - 1, 2 ** 64 - 1)) == (2 ** 64 - 1) * (1 + cv.Z2) % R


@pytest.mark.parametrize("bitrev", [False, True])
def test_facts_by_construction_refuse_what_the_equation_cannot_see(bitrev):
    b = cv.valid_batch((4, 2, 1, bitrev), 5, 0xFAC7 + bitrev)
    assert cv.want(b)
    v = b.cells[2][2][3]
    same = b.with_value(2, 3, v + R)
    assert v + R < 2 ** 256 and cv.holds(same) and not cv.want(same) and not cv.want_each(same)[2]      # the same residue, another input
    assert not cv.want(b.with_cell(1, m=b.cells[1][1] + b.big_m))
    assert not cv.want(b.with_pair(4, 0, 0)) and cv.want(b.with_pair(4, 0, 1)) and cv.want(b.with_pair(4, 1, 0))
    assert not cv.want(b.with_invalid("c", 0, None)) and cv.holds(b.with_invalid("c", 0, None))
    assert cv.want(b.with_rand([(a, 0) for a, _ in b.rand])) and cv.want(b.with_rand([(0, a) for a, _ in b.rand]))


@pytest.mark.parametrize("shape", [(4, 2, 1, True), (4, 2, 1, False), (6, 2, 1, True), (4, 0, 1, False)])
def test_degenerate_batches(shape):
    """the zero polynomial: C and every proof are the identity; a polynomial of degree below l: every proof is, the commitment is not"""
    big_m = 1 << (shape[0] + shape[2] - shape[1])
    zero = cv.poly_data(cv.zero_polynomial(shape), shape)
    assert zero[0] == 0 and not any(zero[2]) and not any(v for row in zero[1] for v in row)
    low = cv.poly_data(cv.low_degree_polynomial(shape, 0x10), shape)
    assert low[0] != 0 and not any(low[2]) and shape[1] < shape[0]
    polys = [cv.zero_polynomial(shape), cv.low_degree_polynomial(shape, 0x10), [random.Random(3).randrange(R) for _ in range(1 << shape[0])]]
    b = cv.batch_of(polys, [(2, 1), (0, 0), (1, big_m - 1), (0, 3), (2, 0)], shape, 0x11)
    assert cv.want(b) and all(cv.want_each(b))
    assert not cv.want(b.with_value(1, 0, 1)) and not cv.want(b.with_cell(2, c=0)) and not cv.want(b.with_cell(0, c=0))


def test_invalid_points_that_leave_the_equation_alone():
    """what test_gpu_cell_verify.py builds to pin the status bytes: P + T under a scalar the order of T divides is [r] P, and a monomial
    position is idle when coefficient i of every interpolant is zero"""
    import bls12_381_model as bm
    import outside_groups as og
    rng = random.Random(0x70)
    fixtures = og.data()["g1"]
    small = {k: (tuple(int(h, 16) for h in v["p"]), v["order"]) for k, v in fixtures.items() if v["on_curve"] and v["order"]}
    assert {"order3", "order11"} <= set(small)
    p = bm.g1_mul(bm.G1_GEN, rng.getrandbits(64))
    for name in ("order3", "order11"):
        t, h = small[name]
        assert bm.g1_mul(t, h) is None and bm.g1_on_curve(t)
        (a, b), = cv.pairs_divisible_by(rng, 1, h)
        r = cv.scalar((a, b))
        q = bm.g1_add(p, t)
        assert r == a + b * cv.Z2 and r % h == 0 and bm.g1_on_curve(q) and not bm.g1_torsion_free(q)
        assert bm.g1_mul(q, r) == bm.g1_mul(p, r) and bm.g1_mul(q, r + 1) != bm.g1_mul(p, r + 1), name
    for bitrev in (False, True):
        shape = (4, 2, 1, bitrev)
        assert cm.coset_shift(0, 4, 2, 1, bitrev) == 1                                 # a cell of index 0: r c^l = r
        for keep in ({1, 2}, {0, 2}):
            polys = [cv.sparse_low_degree_polynomial(shape, 0x71 + j, keep) for j in range(2)]
            b = cv.batch_of(polys, [(0, 0), (1, 3), (1, 7)], shape, 0x72)
            assert cv.want(b) and not any(c[3] for c in b.cells)
            for c, m, vals, _ in b.cells:
                coef = cm.interpolant_coefficients(vals, m, *shape)
                assert [i for i in range(4) if coef[i]] == sorted(keep)


# ------------------------------------------------------------------------------------------------------------------- the planners
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """name -> the figures the planner program prints for the shape"""
    exe = str(tmp_path_factory.mktemp("cell_verify_plan") / "cell_verify_plan_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         "-o", exe, os.path.join(ROOT, "tests", "cell_verify_plan_check.cpp")], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    names = sorted(cv.GPU_SHAPES)
    out = subprocess.run([exe], input="".join("%d %d %d\n" % cv.GPU_SHAPES[k] for k in names), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    assert "cell verify plan_check ok: %d shapes" % len(names) in out.stdout
    print(out.stdout)
    keys = ("log2_d", "log2_l", "n", "tw", "rows", "tiles", "parts", "last_rows", "passes_natural", "ws_natural", "passes_bitrev", "ws_bitrev", "layouts")
    rows = [dict(zip(keys, (int(x) for x in line.split()))) for line in out.stdout.split("\n") if re.match(r"\d+ \d+ \d+  ", line)]
    assert [(r["log2_d"], r["log2_l"], r["n"]) for r in rows] == [cv.GPU_SHAPES[k] for k in names]
    return dict(zip(names, rows))


def test_the_gpu_shapes_reach_the_paths_they_are_named_for(plan):
    for name, p in plan.items():
        log2_d, log2_l, n = cv.GPU_SHAPES[name]
        assert log2_l <= log2_d and p["tw"] == min(1 << log2_l, 64) and p["rows"] == 256 // p["tw"] and p["parts"] == -(-n // p["rows"]), name
        assert p["layouts"] == 8, name                    # both orders x four flag combinations: increasing, 256-aligned, wide enough
    parts, one, tiles, big = plan["S-parts"], plan["S-one"], plan["S-tiles"], plan["S-big"]
    assert (parts["rows"], parts["parts"], parts["last_rows"], parts["tiles"]) == (64, 3, 2, 1)
    assert (one["rows"], one["parts"], one["last_rows"], one["tiles"]) == (256, 2, 44, 1)
    assert (tiles["rows"], tiles["parts"], tiles["last_rows"], tiles["tiles"]) == (4, 3, 1, 2)
    assert (big["rows"], big["parts"], big["last_rows"], big["tiles"]) == (4, 2, 2, 32)
    # above one tile of the transform: more than one pass in both orders; only the natural order ends in a top pass, which reads a workspace
    assert big["passes_natural"] >= 2 and big["passes_bitrev"] >= 2 and big["ws_natural"] == 6 * 2048 * 32 and big["ws_bitrev"] == 0
    for name in ("S-parts", "S-one", "S-tiles", "S-m1-l8", "S-m1-l1", "S-inf", "S-outside", "S-mixed-l16"):
        assert plan[name]["passes_natural"] == plan[name]["passes_bitrev"] == 1 and plan[name]["ws_natural"] == 0, name
    mixed = plan["S-mixed-l16"]
    assert (mixed["rows"], mixed["parts"], mixed["last_rows"]) == (16, 2, 4)
    for name in ("S-m1-l8", "S-m1-l1"):
        assert cv.GPU_SHAPES[name][0] == cv.GPU_SHAPES[name][1] and cv.gpu_batch(name, True).big_m == 1
    assert len({(c, m) for c, m, _, _ in cv.gpu_batch("S-one", True).cells}) == 64        # every cell of both polynomials, so 236 repeats
    with open(os.path.join(CSRC, "zkp_cells.hip")) as f:
        text = f.read()
    # the driver asks the same planners the program asked
    assert "g16::fold_plan(n, l)" in text and "poly::ntt_workspace_bytes(n, b.log2_l, nflags)" in text and "cells::verify_layout(n, b.log2_l, flags," in text


@pytest.mark.parametrize("name", [k for k in sorted(cv.GPU_SHAPES) if k != "S-big"])
def test_the_valid_batches_of_the_gpu_shapes_hold_on_the_model(name):
    for bitrev in (False, True):
        b = cv.gpu_batch(name, bitrev)
        assert b.n == cv.GPU_SHAPES[name][2] and b.log2_d == cv.GPU_SHAPES[name][0] and cv.want(b), (name, bitrev)
        if b.log2_l <= 4:
            assert all(cv.want_each(b.take(range(min(b.n, 6))))), (name, bitrev)
