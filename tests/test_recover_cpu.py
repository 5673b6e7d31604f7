"""CPU gate for the cell recovery (include/zkp_recover.h): the model on Python integers (tests/recover_model.py: the pipeline of the
header) against the DEFINITION - the cells as evaluations on cosets, erase, recover, equal to f; the underdetermined and the corrupted
cases against Lagrange's formula; the planner (csrc/zkp_recover_plan.hpp) walked to the ABI maxima under ASan and UBSan
(tests/recover_plan_check.cpp, a child process); the two kernels' own text on host threads under the same sanitizers
(tests/recover_kernel_host.cpp) against the model's bytes at every column size, and on single-coefficient forgeries
(tests/recover_forgeries.py: every column, every tail position) and on mask bytes other than 1; the new header, the ctypes table and the Rust file against one another; the
replay table against the header; the new kernels' registers."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import cells_model as cm
import poly_model as pm
import recover_model as rm
import recover_shapes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "zkp_recover.h")
RUST = os.path.join(ROOT, "integration", "rust", "src", "recover.rs")
R = pm.R
NEW = ["zkp_das_recover_batch", "zkp_das_recover_batch_dev"]
NAMES = r"zkp_das_recover"


def erased(cells, present):
    """what a client holds: the rows of missing cells are gone"""
    return [row if p else None for row, p in zip(cells, present)]


# ------------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("log2_n,log2_l", rs.CPU_SHAPES)
def test_model_recovers_the_polynomial_from_every_pattern(log2_n, log2_l, bitrev):
    rng = random.Random(0x2EC + 16 * log2_n + log2_l + bitrev)
    n, _, _, _, big_m, _ = rm.sizes(log2_n, log2_l)
    f = [rng.randrange(R) for _ in range(n)]
    cells = cm.cell_values(f, log2_n, log2_l, 1, bitrev)                 # the definition: evaluations on the cosets
    assert rm.cells_of(f, log2_n, log2_l, bitrev) == cells              # ... which the tests' transform route reproduces
    for kind in rm.PATTERNS:
        present = rm.pattern(kind, big_m, rng)
        assert sum(present) >= big_m // 2 and (kind in ("none", "one") or sum(present) == big_m // 2), kind
        assert rm.recover(erased(cells, present), present, log2_n, log2_l, bitrev) == (f, 1), (kind, log2_n, log2_l, bitrev)
    for poly in ([0] * n, [R - 1] * n, [0] * (n - 1) + [1]):             # zero, all r - 1, only the top coefficient
        present = rm.pattern("random-half", big_m, rng)
        assert rm.recover(erased(rm.cells_of(poly, log2_n, log2_l, bitrev), present), present, log2_n, log2_l, bitrev) == (poly, 1)


def test_the_patterns_that_make_the_vanishing_polynomial_sparse():
    """every other exponent m' missing gives Z = Y^(M/2) -+ 1: the even and odd cells in natural order, the two halves in the stored
    (bit-reversed) order, where the cells of a half are every other coset"""
    for mu in (1, 3, 5):
        big_m = 1 << mu
        dom = pm.domain(mu)
        for bitrev, kinds in ((False, ("even", "odd")), (True, ("first-half", "second-half"))):
            for kind in kinds:
                present = rm.pattern(kind, big_m)
                missing = [pm.bit_reverse(m, mu) if bitrev else m for m in range(big_m) if not present[m]]
                assert len({mp & 1 for mp in missing}) == 1
                z = rm.vanishing(missing, mu)
                assert [i for i, v in enumerate(z) if v] == [0, big_m // 2] and z[big_m // 2] == 1 and z[0] in (1, R - 1), (mu, bitrev, kind)
                assert all((cm.horner(z, dom[mp]) == 0) == (mp in missing) for mp in range(big_m))
        dense = rm.vanishing([pm.bit_reverse(m, mu) for m in range(big_m) if not rm.pattern("even", big_m)[m]], mu)
        assert mu == 1 or sum(1 for v in dense if v) > 2                 # the same cells in the other order: a dense Z


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("log2_n,log2_l", rs.CPU_SHAPES)
def test_model_on_corrupted_and_on_too_few_cells(log2_n, log2_l, bitrev):
    rng = random.Random(0xBAD + 16 * log2_n + log2_l + bitrev)
    n, l, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
    f = [rng.randrange(R) for _ in range(n)]
    cells = rm.cells_of(f, log2_n, log2_l, bitrev)
    order = list(range(big_m))
    rng.shuffle(order)
    bad = [list(row) for row in cells]
    bad[order[0]][rng.randrange(l)] += 1
    bad[order[0]] = [v % R for v in bad[order[0]]]
    # more than M / 2 cells, one value corrupted: ok = 0
    for keep in sorted({k + 1, big_m}):
        present = [1 if m in order[:keep] else 0 for m in range(big_m)]
        assert rm.recover(erased(bad, present), present, log2_n, log2_l, bitrev)[1] == 0, keep
        assert rm.recover(erased(cells, present), present, log2_n, log2_l, bitrev) == (f, 1)
    # exactly M / 2 cells, one value corrupted: ok = 1 and the OTHER interpolant, which Lagrange's formula names
    present = [1 if m in order[:k] else 0 for m in range(big_m)]
    got, ok = rm.recover(erased(bad, present), present, log2_n, log2_l, bitrev)
    assert ok == 1 and got != f and got == rm.interpolant_of_half(bad, present, log2_n, log2_l, bitrev)
    assert rm.cells_of(got, log2_n, log2_l, bitrev)[order[0]] == bad[order[0]]
    # M / 2 - 1 cells: ok = 0 and a zero row
    present = [1 if m in order[:k - 1] else 0 for m in range(big_m)]
    assert rm.recover(erased(cells, present), present, log2_n, log2_l, bitrev) == ([0] * n, 0)


def test_the_instances_of_the_gpu_tests_are_what_they_claim():
    """tests/recover_replay_cases.py: the kinds, the flags, the garbage in missing cells, the sets of the replay case"""
    import recover_replay_cases as rrc
    inst = rrc.instance(rrc.KINDS, *rs.SMALL, True, 0x51)
    n, l, k, _, big_m, _ = rm.sizes(*rs.SMALL)
    assert inst["ok"].tolist() == [1] * 7 + [0, 1, 0] and inst["free"] == [9]
    pres = inst["present"].reshape(len(rrc.KINDS), big_m)
    assert pres.sum(axis=1).tolist() == [big_m, big_m - 1] + [k] * 5 + [k - 1, k, k + 1]
    vals = inst["values"].reshape(len(rrc.KINDS), big_m, l, 4)
    assert all(not rrc.below_r(vals[j, m]) for j in range(len(rrc.KINDS)) for m in range(big_m) if not pres[j, m])      # nobody may read them
    assert rrc.below_r(vals[pres == 1]) and not inst["coeffs"].reshape(len(rrc.KINDS), -1)[7].any()
    for case in rrc.CASES:
        sets, want = case.make(None, case.shape, 3)
        assert len({s["present"].tobytes() for s in sets}) == 3 and len({w[0].tobytes() for w in want}) == 3
        assert [w[1].tolist() for w in want][1].count(0) == 1            # set B holds the blob with too few cells


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("log2_n,log2_l", rs.CPU_SHAPES)
def test_model_on_single_coefficient_forgeries(log2_n, log2_l, bitrev):
    """f + a X^(i0 + l t0), k <= t0 < M, with k + s cells present (tests/recover_forgeries.py): s = 0 is the other interpolant; t0 < k + s
    leaves ONE non-zero tail entry, column i0 at t0, and f below it; t0 >= k + s wraps into the tail entries below k + s of column i0 alone"""
    import recover_forgeries as rf
    rng = random.Random(0xF06 + 16 * log2_n + log2_l + bitrev)
    n, l, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
    f = [rng.randrange(R) for _ in range(n)]
    cells = rm.cells_of(f, log2_n, log2_l, bitrev)
    assert rf.forge([[0] * l] * big_m, 1, n - 1, log2_n, log2_l, bitrev) == rm.cells_of([0] * (n - 1) + [1], log2_n, log2_l, bitrev)
    lagrange = 0
    for s in sorted({0, 1, 2, k} & set(range(k + 1))):
        for i0, t0, e in rf.tail_exps(log2_n, log2_l):
            present = rf.keep_cells(big_m, k + s, rng)
            bad = rf.forge(cells, 1 + rng.randrange(R - 1), e, log2_n, log2_l, bitrev)
            cols = rm.decode(erased(bad, present), present, log2_n, log2_l, bitrev)
            tail = {(i, t) for i in range(l) for t in range(k, big_m) if cols[i][t]}
            got, ok = rm.recover(erased(bad, present), present, log2_n, log2_l, bitrev)
            if s == 0:
                assert not tail and ok == 1 and got != f, (s, i0, t0)
                if lagrange < 2:                                         # Lagrange's formula is cubic: twice per shape
                    assert got == rm.interpolant_of_half(bad, present, log2_n, log2_l, bitrev)
                    lagrange += 1
            elif t0 < k + s:
                assert tail == {(i0, t0)} and ok == 0 and got == f, (s, i0, t0)
            else:
                assert tail and {i for i, _ in tail} == {i0} and ok == 0, (s, i0, t0)
                assert all(got[i + l * t] == f[i + l * t] for i in range(l) if i != i0 for t in range(k)), (s, i0, t0)
                # the decode has degree below k + s: s tail entries to wrap into (Y^t0 modulo the present cells' vanishing polynomial,
                # whose coefficients are symmetric functions of roots of unity: some of them may vanish)
                assert all(t < k + s for _, t in tail), (s, i0, t0)


def test_the_forgery_instances_are_what_they_claim():
    """tests/recover_forgeries.py: the gathered monomials against the transform, the fast canonical test against the slow one, the sweeps'
    cover of every tail position, the edge lanes' coefficients against the planner's tile, the instances of the contracts"""
    import recover_forgeries as rf
    import recover_replay_cases as rrc
    from replay_cases import fr_rows
    for (log2_n, log2_l), bitrev in [((4, 2), False), ((4, 2), True), ((5, 0), True), ((3, 3), False), ((3, 3), True), ((6, 3), True)]:
        n = 1 << log2_n
        exps = [0, 1, n - 1, n, 2 * n - 1, n + 3]
        got = rf.monomial_cells(exps, log2_n, log2_l, bitrev)
        for j, e in enumerate(exps):
            f = [1 if d == e else 0 for d in range(2 * n)]                # as a polynomial of degree below D: its D evaluations, cut into cells
            ev = pm.ntt(f, log2_n + 1, bitrev=bitrev)
            l, big_m = 1 << log2_l, 2 * n >> log2_l
            cells = [ev[l * m:l * m + l] for m in range(big_m)] if bitrev else [[ev[m + big_m * u] for u in range(l)] for m in range(big_m)]
            assert got[j].tobytes() == fr_rows([v for row in cells for v in row]).tobytes(), (log2_n, log2_l, bitrev, e)
            assert cells == rf.monomial_rows(e, log2_n, log2_l, bitrev)
            if e < n:
                assert cells == rm.cells_of(f[:n], log2_n, log2_l, bitrev)
    edge = fr_rows([0, R - 1, R, R + 1, (1 << 256) - 1, R - (1 << 64), R + (1 << 64), R - (1 << 192), R + (1 << 192)])
    for j in range(len(edge)):
        assert rf.canonical(edge[j]) == rrc.below_r(edge[j]) == (j in (0, 1, 5, 7)), j
    assert not rf.canonical(edge) and rf.canonical(edge[[0, 1, 5, 7]]) and not rf.canonical(np.full((3, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
    for log2_n, log2_l, cols in rs.FORGERY_SWEEPS:
        n, l, k, _, big_m, mu = rm.sizes(log2_n, log2_l)
        tails = rf.tail_exps(log2_n, log2_l, cols)
        assert {(i0, t0) for i0, t0, _ in tails} == {(i0, t0) for i0 in (cols or range(l)) for t0 in range(k, big_m)}      # no tail position left out
        assert all(e == i0 + l * t0 and n <= e < 2 * n for i0, t0, e in tails) and (0, k, n) in tails
        twins = rf.twin_exps(log2_n, log2_l)
        assert n - 1 in twins and max(twins) == n - 1 and len([e for e in twins if e % 8 == 5 * (e // 8) % 8]) >= n // 8
        # the edge lanes: elements q + 256 u of the tile the planner describes (c = e mod 2^cl, p = e >> cl), in every workgroup
        cl, c_wg = 10 - mu, min(l, 1 << (10 - mu))
        for g in range(l // c_wg):
            for e in (0, 255, 256, 511, 512, 767, 768, 1023):
                c, t = e & ((1 << cl) - 1), pm.bit_reverse(e >> cl, mu)
                if c < c_wg and t < k:
                    assert g * c_wg + c + l * t in rf.edge_lane_exps(log2_n, log2_l)
        assert rf.edge_lane_exps(log2_n, log2_l) and set(rf.edge_lane_exps(log2_n, log2_l)) <= set(twins)
    assert rs.FORGERY_SWEEPS[3][2] == (0, 7, 8, 63)                        # PeerDAS: 8 columns per workgroup, 64 columns
    inst = rf.sweep(6, 3, True)
    n_f, n_t = 64, len(rf.twin_exps(6, 3))
    assert inst["ok"].size == n_f + n_t and inst["ok"].sum() == n_t and len(inst["free"]) == n_f and inst["present"].all()
    assert (inst["ok"] == (inst["exps"] < 64)).all() and sorted(inst["exps"][inst["free"]].tolist()) == list(range(64, 128))
    assert np.count_nonzero(np.diff(inst["ok"])) >= 8                      # good blobs stand between forged ones
    co = inst["coeffs"].reshape(n_f + n_t, 64, 4)
    for j in np.nonzero(inst["ok"])[0]:
        assert co[j].sum() == 1 and co[j, inst["exps"][j], 0] == 1
    # the contracts
    small = rrc.instance(("random-half", "few", "one"), *rs.SMALL, True, 0x3A5)
    other = rf.other_mask_bytes(small)
    assert other["present"].tobytes() != small["present"].tobytes() and other["values"] is small["values"] and set(other["present"].tolist()) == {0, 1, 2, 0x80, 0xFF}
    mixed = rf.mixed_instance(*rs.SMALL, True)
    assert mixed["ok"].tolist() == [0, 1, 0, 0, 1, 0, 1, 0] and mixed["free"] == [2, 5]
    assert not mixed["coeffs"].reshape(8, -1)[[0, 3, 7]].any() and mixed["coeffs"].reshape(8, -1)[[1, 4, 6]].any(axis=1).all()
    st = rf.structured_instance(*rs.SMALL, False)
    n_co, _, k, _, big_m, _ = rm.sizes(*rs.SMALL)
    zero = [j for j, name in enumerate(st["labels"]) if name.startswith("zero")]
    assert len(zero) == 8 and st["ok"][zero].tolist() == [1] * 5 + [0] + [1] * 2 and not st["coeffs"].reshape(-1, n_co * 4)[zero].any() and not st["free"]
    assert st["present"].reshape(-1, big_m)[zero[-2:]].sum(axis=1).tolist() == [k, k]
    assert len(rf.STRUCTURED) == 19 and max(rf.STRUCTURED) == R - 1 and len(set(rf.STRUCTURED)) == 19 and all(v < R for v in rf.STRUCTURED)
    lim = rf.limit_instance(*rs.LIMIT, rs.LIMIT_MISSING, True)
    gone = (lim["present"].reshape(-1, 1024) == 0).sum(axis=1).tolist()
    assert gone == list(rs.LIMIT_MISSING) + [512, 512] and lim["ok"].tolist() == [1 if g <= 512 else 0 for g in gone] and not lim["free"]
    assert {1024 - g for g in gone} >= {1024, 1023, 769, 768, 767, 683, 513, 512, 511}


# ------------------------------------------------------------------------------------------------------------------- the planner
def _clean(out):
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("recover_plan") / "recover_plan_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         "-o", exe, os.path.join(ROOT, "tests", "recover_plan_check.cpp")], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def test_planner_holds_at_the_abi_maxima(plan_exe):
    out = subprocess.run([plan_exe], capture_output=True, text=True, timeout=900)
    _clean(out)
    assert re.search(r"recover plan_check ok: \d+ cases", out.stdout)
    for src, inc in (("zkp_recover.hip", "zkp_recover.hpp"), ("zkp_recover.hip", "zkp_recover_plan.hpp"), ("zkp_pairings.hip", "zkp_recover.hpp"),
                     ("zkp_recover.hpp", "zkp_recover_plan.hpp")):
        with open(os.path.join(CSRC, src)) as f:
            assert '#include "%s"' % inc in f.read(), src
    with open(os.path.join(CSRC, "zkp_recover_plan.hpp")) as f:
        text = f.read()
    assert "hip_runtime" not in text and "getenv" not in text          # host-only text, and no knob


def test_the_shapes_of_the_gpu_tests_reach_what_they_claim(plan_exe):
    """the planner's own answer for tests/recover_shapes.py: the columns of a workgroup, the slice length of the sliced call"""
    shapes = [(n, a, b) for a, b, n, _ in rs.GPU_SHAPES] + [(rs.SLICE_N, rs.SLICE_LOG2_N, rs.SLICE_LOG2_L)]
    out = subprocess.run([plan_exe, "shapes"], input="".join("%d %d %d\n" % s for s in shapes), capture_output=True, text=True, timeout=900)
    _clean(out)
    rows = [tuple(int(x) for x in line.split()) for line in out.stdout.split("\n") if line]
    assert [r[:3] for r in rows] == shapes
    by = {(r[1], r[2]): r[3:] for r in rows}
    assert by[(1, 1)][1:] == (2, 1) and by[(4, 0)][1:] == (1, 1)                       # M = 2: l columns of 512 slots; l = 1
    assert by[(4, 2)][1:] == (4, 1)                                                    # fewer columns (4) than the tile has slots (128)
    assert by[(10, 1)][1:] == (1, 2)                                                   # M = 1024: one column fills the tile
    assert by[(12, 6)][1:] == (8, 8)                                                   # PeerDAS: 8 columns, runs of 256 B
    assert by[(11, 11)][1:] == (512, 4)
    assert by[(rs.SLICE_LOG2_N, rs.SLICE_LOG2_L)][0] == rs.SLICE_LEN == (1 << 21) >> (rs.SLICE_LOG2_N + 1)
    with open(HEADER) as f:
        assert "floor(2^21 / D)" in f.read()
    # every column size: the table states mu, cl, the columns of a workgroup and the workgroups of a blob; the planner confirms each row
    want = list(rs.EVERY_MU) + [(6, 3, 4, 6, 8, 1), (10, 2, 9, 1, 2, 2), (10, 1, 10, 0, 1, 2), (12, 6, 7, 3, 8, 8), (4, 2, 3, 7, 4, 1), (10, 10, 1, 9, 512, 2)]
    assert [w[:2] for w in want[len(rs.EVERY_MU):]] == [s[:2] for s in rs.FORGERY_SWEEPS] + [rs.SMALL, rs.FORGERY_HOST_GROUPS]
    assert rs.LIMIT == (10, 1) and set(rs.FORGERY_ERASED) == {(6, 3), rs.SMALL}
    out = subprocess.run([plan_exe, "tiles"], input="".join("%d %d\n" % w[:2] for w in want), capture_output=True, text=True, timeout=900)
    _clean(out)
    assert [tuple(int(x) for x in line.split()) for line in out.stdout.split("\n") if line] == want
    assert len(set(rs.EVERY_MU)) == len(rs.EVERY_MU) and {w[2] for w in rs.EVERY_MU} == set(range(1, 11))
    for log2_n, log2_l, mu, cl, cols, groups in rs.EVERY_MU:
        assert mu == log2_n + 1 - log2_l and cl == 10 - mu and log2_n + 1 <= 13, (log2_n, log2_l)
    for mu in range(1, 11):
        rows = [w for w in rs.EVERY_MU if w[2] == mu]
        assert {w[1] for w in rows} == {0, 1, 3, 11 - mu}, mu                          # l = 1, 2, 8 and 2^(cl + 1)
        assert any(w[5] >= 2 and w[4] == 1 << w[3] for w in rows), mu                  # two workgroups or more, every column slot taken
        assert mu == 10 or any(w[4] < 1 << w[3] for w in rows), mu                     # idle column slots (M = 1024: the tile is ONE column)
    assert {w[2] for w in rs.EVERY_MU if w[3] in (1, 2) and w[5] >= 2} == {8, 9}      # M = 256 and M = 512 with more than one workgroup


def test_the_sliced_call_of_the_gpu_test_crosses_a_slice_boundary():
    """two slices with a short last one; rows behind the boundary differ from the rows at offset 0, and the expected bytes read with a
    wrong offset differ in both output arrays (tests/slice_pools.py)"""
    import recover_replay_cases as rrc
    import slice_pools as sp
    for bitrev in (False, True):
        call = rrc.slice_call(bitrev)
        assert call.starts == [0, rs.SLICE_LEN] and call.tail == 3 and set(call.idx[-3:]) == set(rrc.SLICE_TAIL) and not set(call.idx[:-3]) & set(rrc.SLICE_TAIL)
        w = sp.window(call, call.starts[1])
        for name, (arr, per) in list(call.inputs.items()) + list(call.outputs.items()):
            assert sp.rows(arr, per, call.starts[1], w).tobytes() != sp.rows(arr, per, 0, w).tobytes(), name
        for name in call.outputs:
            for how in ("zero", "previous"):
                assert sp.reading(call, name, how).tobytes() != call.want(name).tobytes(), (name, how)
        assert not call.pool["free"] and 0 in call.pool["ok"] and 1 in call.pool["ok"]


# ------------------------------------------------------------------------------------------------------------------- the kernels' own text
@pytest.fixture(scope="module")
def kernel_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("recover_kernels") / "recover_kernel_host")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                         "-Wno-unknown-pragmas", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "recover_kernel_host.cpp")], capture_output=True, text=True,
                        timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("log2_n,log2_l,n", rs.KERNEL_HOST_SHAPES)
def test_kernels_on_host_threads_equal_the_model(kernel_exe, tmp_path, log2_n, log2_l, n, bitrev):
    """k_rec_vanish, k_rec_zinv and k_rec_column as written in zkp_recover.hip, one host thread per lane: every M = 2^mu, mu = 1 .. 10, with l = 1
    and l = 4 (every round schedule of column_transform, every count of column slots); what the driver's borrowed transform computes in between (the cells' inverse transforms, Z on the roots and on the coset)
    comes from the model.  The third blob of a case has too few cells, missing cells hold bytes above r"""
    import recover_replay_cases as rrc
    n_co, l, k, _, big_m, mu = rm.sizes(log2_n, log2_l)
    rng = random.Random(0x4057 + 16 * log2_n + log2_l + bitrev)
    kinds = ("random-half", "even", "few")[:n]
    pres_b, coef_b, zr_b, zs_b, want_zc, want_zi, want_f, want_ok = b"", b"", b"", b"", [], [], [], []
    for kind in kinds:
        rows, present, want, ok = rrc.blob(kind, log2_n, log2_l, bitrev, rng)
        mp = [pm.bit_reverse(m, mu) if bitrev else m for m in range(big_m)]
        z = rm.vanishing([mp[m] for m in range(big_m) if not present[m]], mu) if ok else [0] * big_m
        pres_b += bytes(present)
        for m in range(big_m):
            coef_b += pm.to_bytes(pm.ntt(rows[m], log2_l, inverse=True, bitrev=bitrev) if present[m] else rows[m])
        zr_b += pm.to_bytes(pm.ntt(z, mu))
        zs = pm.ntt(z, mu, coset=True)
        zs_b += pm.to_bytes(zs)
        want_zi += [pow(v, -1, R) if v else 0 for v in zs]
        want_zc += z
        want_f += want
        want_ok.append(ok)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(pres_b + coef_b + zr_b + zs_b)
    out = subprocess.run([kernel_exe, str(fin), str(fout), str(log2_n), str(log2_l), str(n), str(int(bitrev))], capture_output=True, text=True, timeout=900)
    _clean(out)
    raw = fout.read_bytes()
    flags = b"".join(v.to_bytes(4, "little") for v in want_ok)
    assert len(raw) == 2 * 32 * n * big_m + 4 * n + 32 * n * n_co + 4 * n
    at = 32 * n * big_m
    assert raw[:at] == pm.to_bytes(want_zc), "the coefficients of Z"
    assert raw[at:at + 4 * n] == flags, "ok after k_rec_vanish"
    assert raw[at + 4 * n:2 * at + 4 * n] == pm.to_bytes(want_zi), "1 / Z on the coset"
    at = 2 * at + 4 * n
    assert raw[at:at + 32 * n * n_co] == pm.to_bytes(want_f), "the recovered coefficients"
    assert raw[-4 * n:] == flags, "ok after k_rec_column"


def test_the_column_kernel_flags_inconsistent_cells_on_host_threads(kernel_exe, tmp_path):
    """more than M / 2 cells and one corrupted value: k_rec_column stores ok = 0, and what it leaves in the row is canonical"""
    import recover_replay_cases as rrc
    log2_n, log2_l, bitrev = 4, 2, True
    n_co, l, k, _, big_m, mu = rm.sizes(log2_n, log2_l)
    rows, present, want, ok = rrc.blob("more-bad", log2_n, log2_l, bitrev, random.Random(0x1C0))
    assert want is None and ok == 0
    z = rm.vanishing([pm.bit_reverse(m, mu) for m in range(big_m) if not present[m]], mu)
    data = bytes(present) + b"".join(pm.to_bytes(pm.ntt(rows[m], log2_l, inverse=True, bitrev=True) if present[m] else rows[m]) for m in range(big_m))
    data += pm.to_bytes(pm.ntt(z, mu)) + pm.to_bytes(pm.ntt(z, mu, coset=True))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(data)
    out = subprocess.run([kernel_exe, str(fin), str(fout), str(log2_n), str(log2_l), "1", "1"], capture_output=True, text=True, timeout=900)
    _clean(out)
    raw = fout.read_bytes()
    at = 32 * big_m
    assert raw[at:at + 4] == (1).to_bytes(4, "little") and raw[-4:] == (0).to_bytes(4, "little")
    assert all(v < R for v in pm.from_bytes(raw[2 * at + 4:-4]))


def _kernels_on_host_threads(kernel_exe, tmp_path, inst, log2_n, log2_l, bitrev, what):
    """an instance through the three kernels on host threads: the flags k_rec_vanish leaves (enough cells), then rows and flags as the
    instance states them"""
    import recover_forgeries as rf
    data, enough = rf.kernel_host_input(inst, log2_n, log2_l, bitrev)
    n = inst["ok"].size
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(data)
    out = subprocess.run([kernel_exe, str(fin), str(fout), str(log2_n), str(log2_l), str(n), str(int(bitrev))], capture_output=True, text=True, timeout=900)
    _clean(out)
    ok_vanish, co, ok = rf.kernel_host_output(fout.read_bytes(), n, log2_n, log2_l)
    assert ok_vanish.tolist() == enough.tolist(), what
    rf.check(co, ok, inst, what)


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("log2_n,log2_l", rs.FORGERY_ERASED + [rs.FORGERY_HOST_GROUPS])
def test_the_column_kernel_flags_every_single_coefficient_forgery_on_host_threads(kernel_exe, tmp_path, log2_n, log2_l, bitrev):
    """X^(i0 + l t0) for EVERY column i0 and EVERY tail position t0 with all cells present - one non-zero element of the decoded tails, in
    one lane of one workgroup - between monomials below N, which come back as unit rows with ok = 1 (X^(N-1) accepted, X^N refused: the
    boundary of the tail); then the same sweep on a random polynomial with a random factor and the last cell missing.  (4, 2) and (6, 3)
    have one workgroup per blob, (10, 10) two: there a forgery of the second workgroup's columns is one the first never sees"""
    import recover_forgeries as rf
    cols = (0, 511, 512, 1023) if (log2_n, log2_l) == rs.FORGERY_HOST_GROUPS else None
    inst = rf.sweep(log2_n, log2_l, bitrev, cols)
    if cols:                                                             # 4 forgeries; of the twins the first 12 beside them
        keep = sorted(inst["free"] + np.nonzero(inst["ok"])[0][:12].tolist())
        n_co, d = 1 << log2_n, 2 << log2_n
        inst = dict(values=inst["values"].reshape(-1, d, 4)[keep].reshape(-1, 4), present=inst["present"].reshape(-1, 2)[keep].reshape(-1),
                    coeffs=inst["coeffs"].reshape(-1, n_co, 4)[keep].reshape(-1, 4), ok=inst["ok"][keep], free=[keep.index(j) for j in inst["free"]],
                    labels=[inst["labels"][j] for j in keep])
        assert len(inst["free"]) == 4 and inst["ok"].tolist().count(1) == 12
    _kernels_on_host_threads(kernel_exe, tmp_path, inst, log2_n, log2_l, bitrev, "all cells present")
    if not cols:
        _kernels_on_host_threads(kernel_exe, tmp_path, rf.erased_sweep(log2_n, log2_l, bitrev, "one"), log2_n, log2_l, bitrev, "the last cell missing")


@pytest.mark.parametrize("bitrev", [False, True])
def test_any_non_zero_mask_byte_is_a_present_cell_on_host_threads(kernel_exe, tmp_path, bitrev):
    """present[j][m] = 2, 0x80 or 0xFF where it was 1: the three kernels, which each read the mask, leave what they left - the count of a
    blob with too few cells is a count of CELLS, not a sum of bytes"""
    import recover_forgeries as rf
    import recover_replay_cases as rrc
    inst = rrc.instance(("few", "random-half", "one", "few", "none", "half-bad"), *rs.SMALL, bitrev, 0x3A5)
    assert inst["ok"].tolist() == [0, 1, 1, 0, 1, 1]
    other = rf.other_mask_bytes(inst)
    n, big_m = 6, 2 << (rs.SMALL[0] - rs.SMALL[1])
    assert (other["present"].reshape(n, big_m).astype(np.int64).sum(axis=1)[[0, 3]] >= big_m // 2).all()      # a sum of bytes would call them enough
    _kernels_on_host_threads(kernel_exe, tmp_path, other, *rs.SMALL, bitrev, "mask bytes")


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
    assert sorted(c) == sorted(NEW) == sorted(_lib.RECOVER_SIGNATURES)
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
    for name, (res, args) in _lib.RECOVER_SIGNATURES.items():
        assert (ckind(res), [ckind(x) for x in args]) == c[name], (name, "ctypes")
        assert getattr(lib, name).argtypes == args                                   # load() bound the sixth table as well
    tables = [_lib.SIGNATURES, _lib.POLY_SIGNATURES, _lib.PROVE_SIGNATURES, _lib.FK20_SIGNATURES, _lib.CELLS_SIGNATURES, _lib.RECOVER_SIGNATURES]
    assert sum(len(t) for t in tables) == len(set().union(*tables))                  # the six tables are disjoint
    assert lib.zkp_abi_version() == 4


def test_the_old_boundary_gained_one_comment_and_one_module_line():
    with open(os.path.join(ROOT, "include", "zkp_pairings.h")) as f:
        old = f.read()
    assert old.count("zkp_recover.h") == 1 and not re.search(NAMES, old)
    line = [x for x in old.split("\n") if "zkp_recover.h" in x][0]
    assert line.startswith("/*") and line.endswith("*/") and not re.search(r"zkp_[a-z0-9_]+\(|zkp_(poly|prove|fk20|cells)\.h", line)
    for other in ("zkp_poly.h", "zkp_prove.h", "zkp_fk20.h", "zkp_cells.h"):
        with open(os.path.join(ROOT, "include", other)) as f:
            assert not re.search(NAMES + "|zkp_recover", f.read()), other
    with open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")) as f:
        lib_rs = f.read()
    assert len(re.findall(r"^(?:pub )?mod recover;$", lib_rs, re.M)) == 1 and not re.search(NAMES, lib_rs)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert all(x in mk for x in ("zkp_recover.hip", "zkp_recover.hpp", "zkp_recover_plan.hpp", "include/zkp_recover.h"))
    assert os.path.exists(os.path.join(ROOT, "integration", "c", "zkp_recover.c"))
    with open(HEADER) as f:
        h = f.read()
    assert all(x in h for x in ('#include "zkp_cells.h"', "under ABI version 4", "Slices and workspace", "Cost:", "How", "ZKP_ERR_ARG", "never interpreted"))


def test_every_dev_entry_point_of_the_new_header_has_a_replay_case_or_a_written_reason():
    import recover_replay_cases as rrc
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(zkp_\w+_dev)\(", _header_text()))
    table, excluded = rrc.table_c_names(), set(rrc.EXCLUDED)
    assert declared == {n for n in NEW if n.endswith("_dev")}
    assert not (table & excluded)
    assert declared - (table | excluded) == set(), "no replay case and no reason: %s" % sorted(declared - (table | excluded))
    assert (table | excluded) - declared == set(), "not declared in the header: %s" % sorted((table | excluded) - declared)
    assert all(isinstance(why, str) and len(why) > 20 for why in rrc.EXCLUDED.values())
    ids = [c.id for c in rrc.CASES]
    assert len(ids) == len(set(ids))
    from zkvm_pairings_amd.engine import PairingEngine
    for c in rrc.CASES:
        assert c.c_names and callable(getattr(PairingEngine, c.method)) and len(c.shape) == len(c.small), c.id
    assert {c.method for c in rrc.CASES} == {"das_recover"}


def test_new_symbols_refuse_a_null_context_and_the_python_layer_exposes_the_feature():
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    assert lib.zkp_das_recover_batch(None, None, None, 0, 0, 0, 0, None, None) == -1
    assert lib.zkp_das_recover_batch_dev(None, None, None, 0, 0, 0, 0, None, None, None) == -1
    assert callable(z.PairingEngine.das_recover)
    for name in ("recover_polynomials_batch", "recover_cells_and_kzg_proofs_batch"):
        assert callable(getattr(z, name)) and name in z.__all__
    assert callable(z.synthetic.das_recover_instance)


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")), reason="library not built")
def test_new_kernels_are_there_and_do_not_spill():
    from test_codeobject import READELF, _kernels
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_rec_" in n}
    assert len(new) == 4, sorted(new)                                                  # vanish, zinv, column; the validation mode's check
    for part in ("k_rec_vanish", "k_rec_zinv", "k_rec_column", "k_rec_valid"):
        assert sum(part in n for n in new) == 1, part
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgpr"] <= 256, (n, v)
    col = [v for n, v in new.items() if "k_rec_column" in n][0]
    assert col["lds"] == 32768, col                                                    # the tile of zkp_poly_plan.hpp: 2^10 elements of 32 B
    # no name of the new kernels contains what an older gate counts by
    counted = ("k_ntt_pass", "k_msm_", "k_add28", "k_g1_mul_endo28", "k_fr_", "k_kzg_", "k_prove_", "k_spmv", "k_poly_coset", "k_open_quot", "k_rlc_",
               "k_g16_", "k_frinv_", "k_freval_", "k_zero_fill", "k_coop", "k_g1ntt_", "k_fk20_", "k_cell_")
    assert not [n for n in new for x in counted if x in n]
    # the transform the recovery drives kept its registers and LDS
    hit = [v for n, v in k.items() if "k_ntt_passILb0" in n]
    assert len(hit) == 1 and (hit[0]["vgpr"], hit[0]["lds"], hit[0]["spill"], hit[0]["scratch"]) == (155, 32768, 0, 0), hit
