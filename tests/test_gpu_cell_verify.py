"""The batch verifier of the KZG cells on one MI355X (zkp_kzg_cell_verify_batch, include/zkp_cells.h) on batches whose verdict is known
without the library: every batch is built in exponent space (tests/cell_verify_cases.py), every expected verdict is want(batch) - the
combined equation on Python integers ANDed with the facts of the construction.  Forged batches that hold exactly under the scalars
a_j + b_j z^2 and under no others; one bad cell in every part of the fold; values and indices of the same residue that are other inputs;
zero scalars; the zero polynomial, polynomials of degree below l, flagged infinities with stale coordinates; points outside the groups
in every position under every flag combination that still checks them, and invalid points that leave the equation alone; mixed
batches against the per-cell path; a domain table larger than D.  The shapes reach several parts and tiles of the fold and a transform
above one tile (tests/test_cell_verify_cpu.py holds them to the planners).  Run with -m gpu."""
import random

import numpy as np
import pytest

import cell_verify_cases as cv
import outside_groups as og
import replay_cases as rc

pytestmark = pytest.mark.gpu
R = cv.R
ORDERS = [False, True]
ORDER_IDS = ["natural", "bitrev"]
FLAG_SETS = [dict(), dict(points_checked=True, vk_checked=True), dict(points_checked=True), dict(vk_checked=True)]
BOTH = FLAG_SETS[1]


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    """the engine [tau^l] g2 and the 2048 monomial points of S-big are made with"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def call(e, t, b, rand=None, **kw):
    return e.kzg_cell_verify(t["monomial"], t["g2"], t["tau_l_g2"], t["c"], t["index"], t["values"], t["proof"], b.log2_d, b.log2_l, bitrev=b.bitrev,
                             inf_c=t["inf_c"], inf_proof=t["inf_proof"], rand=t["rand"] if rand is None else rand, **kw)


def verdict(e, h, b, **kw):
    return call(e, cv.wire(b, h), b, **kw)


def call_each(e, t, b):
    import zkvm_pairings_amd as z
    return z.kzg_cell_verify_each(t["monomial"], t["g2"], t["tau_l_g2"], t["c"], t["index"], t["values"].reshape(b.n, 1 << b.log2_l, 4), t["proof"], b.log2_d,
                                  bitrev=b.bitrev, engine=e, inf_c=t["inf_c"], inf_proof=t["inf_proof"]).tolist()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.astype(np.int32)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


# ------------------------------------------------------------------------------------------------------------------- 1. valid batches
@pytest.mark.parametrize("name", ["S-parts", "S-one", "S-tiles", "S-big", "S-m1-l8", "S-m1-l1"])
def test_valid_batches_pass_at_every_shape(eng, helper, name):
    for bitrev in ORDERS:
        b = cv.gpu_batch(name, bitrev)
        assert cv.want(b) is True
        t = cv.wire(b, helper)
        if name == "S-big":                                   # the monomial points came from the helper engine: three of them against the oracle
            assert t["monomial"].shape == (2048, 12)
            assert t["monomial"][[0, 1, 2047]].tobytes() == rc.expect_points(1, [1, cv.TAU, pow(cv.TAU, 2047, R)])[0].tobytes()
        if b.big_m == 1:
            assert set(t["index"].tolist()) == {0}
        for flags in FLAG_SETS:
            assert call(eng, t, b, **flags) is True, (name, bitrev, flags)
        if name in ("S-parts", "S-one"):                      # resident tensors: an int32 verdict
            d = {k: to_dev(v) for k, v in t.items()}
            got = call(eng, d, b)
            assert got.shape == (1,) and str(got.dtype) == "torch.int32" and int(got.item()) == 1, (name, bitrev)
            bad = cv.wire(b.with_cell(b.n - 1, c=b.cells[b.n - 1][0] + 1), helper)
            assert int(call(eng, {k: to_dev(v) for k, v in bad.items()}, b).item()) == 0, (name, bitrev)


# ------------------------------------------------------------------------------------------------------------------- 2. the forgeries
@pytest.mark.parametrize("bitrev", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name", ["S-parts", "S-tiles"])
def test_forged_batches_get_the_verdict_of_the_equation(eng, helper, name, bitrev):
    base = cv.gpu_batch(name, bitrev)
    n, l = base.n, 1 << base.log2_l
    rng = random.Random(0xF06E + n + bitrev)
    seen = set()
    for i, j in ((0, n - 1), (n // 2, 1)):
        for what, forged, _ in cv.forgeries(base, i, j, sorted({0, 1, l - 1}), rng):
            where = (name, bitrev, what, i, j)
            assert cv.want(forged) is True
            assert verdict(eng, helper, forged) is True, where                 # under its crafted scalars
            t = cv.wire(forged, helper)
            others = [forged.with_pair(j, b=forged.rand[j][1] ^ 1), forged.with_pair(i, a=forged.rand[i][0] ^ 2), forged.with_rand(eng.rlc_random(n))]
            for k, other in enumerate(others):
                assert cv.want(other) is False
                assert call(eng, t, other, rand=np.array(other.rand, dtype=np.uint64)) is False, (where, k)
            seen |= {True, False}
        plain = cv.shift_commitments(base, i, j, rng.randrange(1, R))
        assert cv.want(plain) is False and verdict(eng, helper, plain) is False, (name, bitrev, i, j)
        fresh = plain.with_rand(eng.rlc_random(n))
        assert verdict(eng, helper, fresh) is cv.want(fresh)
        equal = fresh.with_pair(j, *fresh.rand[i])                                # equal scalars cannot tell: why they are random
        assert cv.want(equal) is True and verdict(eng, helper, equal) is True, (name, bitrev, i, j)
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------------------------- 3. one bad cell
@pytest.mark.parametrize("bitrev", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name", ["S-parts", "S-tiles"])
def test_one_bad_cell_anywhere_fails(eng, helper, name, bitrev):
    base = cv.gpu_batch(name, bitrev)
    n, l = base.n, 1 << base.log2_l
    rows = 256 // min(l, 64)
    assert rows < n and verdict(eng, helper, base) is True

    def refused(b, what, **kw):
        assert cv.want(b) is False, what
        assert verdict(eng, helper, b, **kw) is False, (name, bitrev, what, kw)
    for j in (0, rows - 1, rows, n - 1):                      # the first and the last row of the first part, the first row of the second, the last
        c, m, vals, p = base.cells[j]
        for u in (0, l // 2, l - 1):
            refused(base.with_value(j, u, (vals[u] + 1) % R), ("value", j, u))
        refused(base.with_cell(j, m=m ^ 1), ("index", j))
        refused(base.with_cell(j, p=p + 1), ("proof", j))
        refused(base.with_cell(j, c=c + 1), ("commitment", j))
        for u in (0, l - 1):                                  # the same residue, another input
            assert vals[u] + R < 2 ** 256
            same = base.with_value(j, u, vals[u] + R)
            assert cv.holds(same)
            refused(same, ("value + r", j, u))
            refused(same, ("value + r", j, u), **BOTH)
        refused(base.with_cell(j, m=m + base.big_m), ("index + M", j))


# ------------------------------------------------------------------------------------------------------------------- 4. the scalars' edges
@pytest.mark.parametrize("name,bitrev", [("S-parts", True), ("S-tiles", False)])
def test_scalar_edges(eng, helper, name, bitrev):
    base = cv.gpu_batch(name, bitrev)
    n = base.n
    for j in (0, n // 2, n - 1):
        zero = base.with_pair(j, 0, 0)
        assert cv.want(zero) is False and cv.holds(zero)      # the equation cannot see it: the other cells hold
        assert verdict(eng, helper, zero) is False and verdict(eng, helper, zero, **BOTH) is False, (name, j)
    for b in (base.with_rand([(a, 0) for a, _ in base.rand]), base.with_rand([(0, a) for a, _ in base.rand])):
        assert cv.want(b) is True and verdict(eng, helper, b) is True


# ------------------------------------------------------------------------------------------------------------------- 5. infinities
@pytest.mark.parametrize("bitrev", ORDERS, ids=ORDER_IDS)
def test_infinities(eng, helper, bitrev):
    shape = cv.model_shape("S-inf", bitrev)
    n, big_m = cv.GPU_SHAPES["S-inf"][2], 1 << (shape[0] + shape[2] - shape[1])
    rng = random.Random(0x1F + bitrev)
    polys = [cv.zero_polynomial(shape), cv.low_degree_polynomial(shape, 0x1F0), [rng.randrange(R) for _ in range(1 << shape[0])]]
    assert shape[1] < shape[0]

    def agrees(b, t, expect):
        assert cv.want(b) is expect
        assert call(eng, t, b) is expect
        each = cv.want_each(b)
        assert call_each(eng, t, b) == each and all(each) is expect
    finite = cv.wire(cv.batch_of(polys, [(2, m) for m in range(n)], shape, 0x1F1), helper)
    for zeros in ({2}, {0, 4}, set(range(n))):
        picks = [(0 if j in zeros else 2, (3 * j + 1) % big_m) for j in range(n)]
        b = cv.batch_of(polys, picks, shape, 0x1F2 + len(zeros))
        t = cv.wire(b, helper)
        assert all(t["inf_c"][j] == t["inf_proof"][j] == (j in zeros) for j in range(n)) and not t["values"][[4 * j for j in zeros]].any()
        agrees(b, t, True)
        for j in zeros:                                       # coordinates left stale under the flags: valid finite points
            t["c"][j], t["proof"][j] = finite["c"][j], finite["proof"][(j + 1) % n]
        agrees(b, t, True)
        j = max(zeros)
        agrees(b.with_value(j, 1, 5), cv.wire(b.with_value(j, 1, 5), helper), False)
    low = cv.batch_of(polys, [(1, 0), (2, 5), (1, big_m - 1), (2, 0), (1, 7)], shape, 0x1F5)
    t = cv.wire(low, helper)
    assert t["inf_proof"].tolist() == [1, 0, 1, 0, 1] and not t["inf_c"].any()
    agrees(low, t, True)
    off = low.with_value(2, 3, (low.cells[2][2][3] + 1) % R)  # C no longer agrees with the cell's values
    agrees(off, cv.wire(off, helper), False)
    # a finite commitment flagged infinite on an otherwise valid cell: the flag is what counts
    for j in (0, 3):
        t = cv.wire(low, helper)
        t["inf_c"][j] = 1
        agrees(low.with_cell(j, c=0), t, False)


# ------------------------------------------------------------------------------------------------------------------- 6. points outside the groups
def test_points_outside_the_groups_fail_in_every_position(eng, helper):
    """pins the packing of the status bytes (C | pi | monomial | -g2, [tau^l] g2) in the three layouts that have any"""
    b = cv.gpu_batch("S-outside", True)
    n, l = b.n, 1 << b.log2_l
    assert (n, l) == (3, 4) and verdict(eng, helper, b) is True
    g1s = {k: og.g1_wire(pt) for k, pt in og.g1_points().items()}
    g2s = {k: og.g2_wire(q) for k, q in og.g2_points().items()}
    assert len(g1s) >= 2 and len(g2s) >= 2

    def refused(where, pos, pt, what, **kw):
        bad = b.with_invalid(where, pos, pt)
        assert cv.want(bad) is False and cv.holds(bad)
        assert verdict(eng, helper, bad, **kw) is False, (what, where, pos, kw)
    for name, pt in g1s.items():
        for where in ("c", "proof"):
            for pos in (0, n - 1):
                refused(where, pos, pt, name)
                refused(where, pos, pt, name, vk_checked=True)
        for pos in (0, 1, l - 1):
            refused("monomial", pos, pt, name)
            refused("monomial", pos, pt, name, points_checked=True)
    for name, q in g2s.items():
        for where in ("g2", "tau_l_g2"):
            refused(where, 0, q, name)
            refused(where, 0, q, name, points_checked=True)


def unseen_invalid_batches(helper):
    """(what, batch, the flag that still checks the point, the flag that waives its check) of invalid points that leave the equation alone
    (tests/cell_verify_cases.py): P + T in a commitment and - in cells of index 0 - in a proof, under scalars the order of T divides; any
    fixture in a monomial position whose scalar is zero"""
    fixtures = og.data()["g1"]
    small = {k: tuple(int(h, 16) for h in v["p"]) for k, v in fixtures.items() if k in ("order3", "order11")}
    assert [fixtures[k]["order"] for k in sorted(small)] == [11, 3]
    n = cv.GPU_SHAPES["S-outside"][2]
    for bitrev in ORDERS:
        shape = cv.model_shape("S-outside", bitrev)
        rng = random.Random(0x5747 + bitrev)
        polys = [[rng.randrange(R) for _ in range(1 << shape[0])] for _ in range(2)]
        b = cv.batch_of(polys, [(0, 0), (1, 5), (1, 0)], shape, 0).with_rand(cv.pairs_divisible_by(rng, n, 33))
        yield ("valid", bitrev), b, dict(), dict()
        t = cv.wire(b)
        assert not t["inf_proof"].any() and t["index"].tolist() == [0, 5, 0]
        for where in ("c", "proof"):
            for pos in (0, n - 1):
                for name, torsion in sorted(small.items()):
                    bad = b.with_invalid(where, pos, cv.plus_small_order(t[where][pos], torsion))
                    yield (where, pos, name, bitrev), bad, dict(vk_checked=True), dict(points_checked=True)
        for keep, idle in (({1, 2}, (0, 3)), ({0, 2}, (1, 3))):
            low = cv.batch_of([cv.sparse_low_degree_polynomial(shape, 0x5748 + j, keep) for j in range(2)], [(0, 0), (1, 3), (1, 7)], shape, 0x5749)
            yield ("valid", sorted(keep), bitrev), low, dict(), dict()
            for pos in idle:
                for name, pt in sorted(og.g1_points().items()):
                    bad = low.with_invalid("monomial", pos, og.g1_wire(pt))
                    yield ("monomial", pos, name, bitrev), bad, dict(points_checked=True), dict(vk_checked=True)


def test_invalid_points_the_equation_cannot_see_fail_on_their_status_bytes(eng, helper):
    """A point outside the groups in place of a valid one breaks the equation as well, so the test above would pass without any points
    check.  These leave both MSM sums what they were: only their status byte, read at the right offset, refuses them."""
    seen = 0
    for what, b, checking, _ in unseen_invalid_batches(helper):
        if not b.invalid:
            assert cv.want(b) is True and verdict(eng, helper, b) is True, what
            continue
        assert cv.holds(b) and cv.want(b) is False
        assert verdict(eng, helper, b) is False, what
        assert verdict(eng, helper, b, **checking) is False, (what, checking)
        seen += 1
    assert seen == 2 * (2 * 2 * 2 + 2 * 2 * len(og.g1_points()))


# ------------------------------------------------------------------------------------------------------------------- 7. mixed batches
@pytest.mark.parametrize("name", ["S-parts", "S-mixed-l16"])
def test_batch_verdict_equals_all_of_verify_each_on_mixed_batches(eng, helper, name):
    rng = random.Random(0xEAC1 + len(name))
    seen = set()
    for trial in range(3):
        b = cv.gpu_batch(name, trial % 2 == 1)
        n, l = b.n, 1 << b.log2_l
        bad_c = rng.sample(range(n), (trial + 1) % 3)         # 1, 2, 0 bad commitments
        bad_p = rng.sample(range(n), rng.choice([0, 1]))
        bad_v = rng.sample(range(n), rng.choice([0, 1]))
        plus_r = rng.sample(range(n), rng.choice([0, 1]))
        want = [True] * n
        for j in bad_c:
            b = b.with_cell(j, c=b.cells[j][0] + rng.randrange(1, R))
        for j in bad_p:
            b = b.with_cell(j, p=b.cells[j][3] + rng.randrange(1, R))
        for j in bad_v:
            u = rng.randrange(l)
            b = b.with_value(j, u, (b.cells[j][2][u] + rng.randrange(1, R)) % R)
        for j in plus_r:
            u = rng.randrange(l)
            b = b.with_value(j, u, b.cells[j][2][u] % R + R)
        for j in bad_c + bad_p + bad_v + plus_r:
            want[j] = False                                   # by construction
        assert cv.want_each(b) == want and cv.want(b) is all(want)
        t = cv.wire(b, helper)
        assert call_each(eng, t, b) == want, (name, trial)
        assert call(eng, t, b) is all(want), (name, trial)
        seen.add(all(want))
    assert False in seen


# ------------------------------------------------------------------------------------------------------------------- 8. a larger domain table
def test_a_domain_table_grown_by_an_earlier_call(helper):
    """the table of 2^13 points is there before the first cell: every c^-i and c^l is read with a stride (tshift > 0 in k_cell_scale)"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    try:
        e.fr_ntt(np.zeros((1 << 13, 4), dtype=np.uint64), 13)
        for name in ("S-parts", "S-tiles"):
            for bitrev in ORDERS:
                b = cv.gpu_batch(name, bitrev)
                assert cv.want(b) is True and verdict(e, helper, b) is True, (name, bitrev)
                forged = cv.weighted_commitments(b, 1, b.n - 2, 0x5EED)
                assert cv.want(forged) is True and verdict(e, helper, forged) is True, (name, bitrev)
                other = forged.with_pair(1, a=forged.rand[1][0] ^ 2)
                assert cv.want(other) is False and verdict(e, helper, other) is False, (name, bitrev)
                bad = b.with_value(b.n - 1, (1 << b.log2_l) - 1, (b.cells[b.n - 1][2][-1] + 1) % R)
                assert cv.want(bad) is False and verdict(e, helper, bad) is False, (name, bitrev)
    finally:
        e.close()
