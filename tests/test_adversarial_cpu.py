"""CPU gate for the adversarial operands (tests/adversarial.py, tests/golden/adversarial_operands.json): the pool's structure, the C
oracle against Python integers on the pool (it is the reference of tests/test_gpu_adversarial.py), the bit-accurate models of the
cooperative core (tools/coopgen.py) and of the division-step inversion (tools/safegcd_model.py) on the pool and on the searched
vectors - equal to the big-integer model, no model assertion trips, and no internal quantity above what the JSON records."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import adversarial as adv  # noqa: E402
import bls12_381_model as m  # noqa: E402
import coopgen as cg  # noqa: E402
import gen_adversarial as gen  # noqa: E402
import oracle_lib as o  # noqa: E402
import safegcd_model as sgm  # noqa: E402
from test_coopasm import _check_program  # noqa: E402
from test_gpu_parity import _decompress_model  # noqa: E402

P = m.P
SEARCHED = adv.load_searched()
H = lambda s: int(s, 16)
# derived, not measured: a column is an int64, a limb an int32, the quotient estimate of a renormalisation at most 14
HARD = {"max_col": 1 << 63, "red_col": 1 << 63, "wn_limb": 1 << 31, "q_vred": 15, "q_epi": 15, "q_sq": 15, "reduced": 0.51, "canon_hi": 2.0, "canon_lo": 1.0}


def test_pool_structure():
    classes = {}
    for op in adv.pool():
        assert 0 <= op.v < P, op
        classes.setdefault(op.cls, []).append(op)
    assert set(classes) == {"ends", "limbs", "pow2", "pre28", "pre32"} and all(classes.values())
    assert len(adv.ends()) == 9 and len(adv.powers_of_two()) == 3 * 381
    for g, (w, n) in adv.GEOMETRIES.items():
        assert w * n >= 381 > w * (n - 1)
        assert any(op.name.startswith(g + ":") for op in classes["limbs"])
    for op, pre in zip(adv.structured(), adv.preimages(adv.structured(), adv.R28, "pre28")):
        assert pre.v * adv.R28 % P == op.v
    for op, pre in zip(adv.structured(), adv.preimages(adv.structured(), adv.R32, "pre32")):
        assert pre.v * adv.R32 % P == op.v
    tp = adv.targeted_pairs()
    for nm, t in adv.SUM_TARGETS:
        assert len(tp[nm]) > 1000 and all(0 <= a < P and 0 <= b < P and a + b == t for _, a, b in tp[nm])
    for nm, t in adv.DIFF_TARGETS:
        assert len(tp[nm]) > 1000 and all(0 <= a < P and 0 <= b < P and a - b == t for _, a, b in tp[nm])
    for nm, t in adv.PROD_TARGETS:
        assert len(tp["ab=" + nm]) > 1000 and all(0 <= a < P and 0 <= b < P and a * b % P == t for _, a, b in tp["ab=" + nm])
        assert all(a * a % P == t and a == b for _, a, b in tp["a^2=" + nm])
        assert bool(tp["a^2=" + nm]) == (pow(t, (P - 1) // 2, P) in (0, 1))
    for w in (2, 6, 12):
        for nm, r in adv.records(w):
            assert len(r) == 12 and all(0 <= v < P for v in r) and not any(r[w:]), nm


def test_stored_representatives_on_the_28_bit_core_are_the_structured_values():
    """the R = 2^392 pre-images that survive the check on the emulator: the loaded slot holds the balanced digits of V itself; the
    extreme digit patterns are among them"""
    keep = adv.preimages28_verified()
    assert len(keep) > 400
    names = {op.name for op in keep}
    assert any("balanced-digits+max" in n for n in names) and any("balanced-digits-min" in n for n in names)
    # (a small V is mostly stored as V + p: the load's reduction ends in [0, p + p / 2^11).  f_inv canonicalises its input, so
    # for the division steps EVERY pre-image starts from g = V, kept here or not; the GPU tests run them all)
    assert all(op.v * adv.R28 % P == v.v for op, v in zip(adv.preimages(adv.structured(), adv.R28, "pre28"), adv.structured()))
    assert adv.balanced28(P) == list(cg.P_BAL)


def _fp(v):
    return o.to_limbs(v)


def test_oracle_field_operations_on_the_pool():
    ops = adv.pool()
    sub = adv.ends() + adv.core_values()[:24]
    for k, op in enumerate(ops):
        a = _fp(op.v)
        assert o.from_limbs(o.fp_neg(a)) == (-op.v) % P and o.from_limbs(o.fp_square(a)) == op.v * op.v % P, op
        inv = o.fp_invert(a)
        assert (inv is None) == (op.v == 0) and (inv is None or o.from_limbs(inv) == pow(op.v, -1, P)), op
        r = o.fp_sqrt(a)
        assert (None if r is None else o.from_limbs(r)) == m.fp_sqrt(op.v), op
        for y in (sub if op.cls != "pow2" else sub[:9]):      # pow2 against the ends, as the GPU test pairs it with a subset
            b = _fp(y.v)
            assert o.from_limbs(o.fp_mul(a, b)) == op.v * y.v % P and o.from_limbs(o.fp_add(a, b)) == (op.v + y.v) % P
            assert o.from_limbs(o.fp_sub(a, b)) == (op.v - y.v) % P and o.from_limbs(o.fp_sub(b, a)) == (y.v - op.v) % P
    for tname, lst in adv.targeted_pairs().items():
        for nm, x, y in lst:
            a, b = _fp(x), _fp(y)
            assert o.from_limbs(o.fp_add(a, b)) == (x + y) % P and o.from_limbs(o.fp_sub(a, b)) == (x - y) % P, (tname, nm)
            assert o.from_limbs(o.fp_mul(a, b)) == x * y % P, (tname, nm)


def _rec(r):
    return np.concatenate([o.to_limbs(v) for v in r])


def _flat6(t):
    return [c for pr in t for c in pr]


def test_oracle_tower_functions_on_adversarial_records():
    """every tower function the GPU tests take from the oracle, against the big-integer model"""
    f2 = lambda v: (v[0], v[1])
    f6 = lambda v: ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))
    ints = lambda arr, k: o.arr_to_ints(arr)[:k]
    z = (0, 0)
    r2, r6, r12 = adv.records(2), adv.records(6), adv.records(12)        # the records the GPU tests run, all of them
    for i, (nm, a) in enumerate(r2):
        b = r2[(5 * i + 1) % len(r2)][1]
        A, B = _rec(a), _rec(b)
        assert ints(o.fp2_mul(A[:12], B[:12]), 2) == list(m.f2_mul(f2(a), f2(b))), nm
        assert ints(o.fp2_square(A[:12]), 2) == list(m.f2_sqr(f2(a))), nm
        assert ints(o.fp2_mul_by_nonresidue(A[:12]), 2) == list(m.f2_mul_xi(f2(a))), nm
        inv = o.fp2_invert(A[:12])
        assert (inv is None) == (f2(a) == z) and (inv is None or ints(inv, 2) == list(m.f2_inv(f2(a)))), nm
    for i, (nm, a) in enumerate(r6):
        b = r6[(5 * i + 1) % len(r6)][1]
        A, B = _rec(a), _rec(b)
        assert ints(o.fp6_mul(A[:36], B[:36]), 6) == _flat6(m.f6_mul(f6(a), f6(b))), nm
        assert ints(o.fp6_square(A[:36]), 6) == _flat6(m.f6_mul(f6(a), f6(a))), nm
        assert ints(o.fp6_frobenius_map(A[:36]), 6) == _flat6(m.f6_frob_true(f6(a))), nm
        assert ints(o.fp6_mul_by_nonresidue(A[:36]), 6) == _flat6(m.f6_mul_by_v(f6(a))), nm
        assert ints(o.fp6_mul_by_1(A[:36], B[:12]), 6) == _flat6(m.f6_mul(f6(a), (z, f2(b), z))), nm
        assert ints(o.fp6_mul_by_01(A[:36], B[:12], B[12:24]), 6) == _flat6(m.f6_mul(f6(a), (f2(b), (b[2], b[3]), z))), nm
        inv = o.fp6_invert(A[:36])
        assert (inv is None) == (not any(a[:6])) and (inv is None or ints(inv, 6) == _flat6(m.f6_inv(f6(a)))), nm
    for i, (nm, a) in enumerate(r12):
        b = r12[(5 * i + 1) % len(r12)][1]
        A, B = _rec(a), _rec(b)
        fa, fb = m.f12_from_flat_ints(a), m.f12_from_flat_ints(b)
        assert ints(o.fp12_mul(A, B), 12) == m.f12_flat_ints(m.f12_mul(fa, fb)), nm
        assert ints(o.fp12_square(A), 12) == m.f12_flat_ints(m.f12_sqr(fa)), nm
        assert ints(o.fp12_frobenius_map(A), 12) == m.f12_flat_ints(m.f12_frob(fa)), nm
        assert ints(o.fp12_conjugate(A), 12) == m.f12_flat_ints(m.f12_conj(fa)), nm
        assert ints(o.fp12_mul_by_014(A, B[:12], B[12:24], B[24:36]), 12) == m.f12_flat_ints(m.f12_mul(fa, m._sparse_014(f2(b), (b[2], b[3]), (b[4], b[5])))), nm
        inv = o.fp12_invert(A)
        assert (inv is None) == (not any(a)) and (inv is None or ints(inv, 12) == m.f12_flat_ints(m.f12_inv(fa))), nm
        if any(a):
            g = m.f12_mul(m.f12_conj(fa), m.f12_inv(fa))
            g = m.f12_mul(m.f12_frob(m.f12_frob(g)), g)
            assert ints(o.fp12_cyclotomic_square(_rec(m.f12_flat_ints(g))), 12) == m.f12_flat_ints(m.f12_sqr(g)), nm
    nz = [(nm, a) for nm, a in r12 if any(a)]
    got = o.final_exponentiation_batch(np.stack([_rec(a) for _, a in nz]))
    for (nm, a), g in zip(nz, got):
        assert ints(g, 12) == m.f12_flat_ints(m.final_exponentiation(m.f12_from_flat_ints(a))), nm


def test_oracle_square_roots_on_the_pool():
    """fp_sqrt is pinned with the field operations; Fp2::sqrt on the values the GPU test runs: the square / non-square decision of
    the Python model, and a root that squares back (WHICH root is the reference's algorithm, restated only by the oracle)"""
    import compressed_model as cm
    core = adv.core_values()
    for k, op in enumerate(core):
        nxt = core[(k + 1) % len(core)]
        for v in ((op.v, 0), (0, op.v), (op.v, op.v), (op.v, nxt.v)):
            for w in (v, m.f2_sqr(v)):
                r = o.fp2_sqrt(np.concatenate([_fp(w[0]), _fp(w[1])]))
                assert (r is None) == (cm.fp2_sqrt_fast(w) is None), (op, w)
                if r is not None:
                    ri = o.arr_to_ints(r)
                    assert m.f2_sqr((ri[0], ri[1])) == w, (op, w)


# ---- the 28-bit cooperative core on the emulator -------------------------------------------------------------------------------
def _model(name, a, b):
    """the big-integer value of a tower program (what run_program must return)"""
    f2 = lambda v: (v[0], v[1])
    f6 = lambda v: ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))
    pad = lambda v: list(v) + [0] * (12 - len(v))
    z = (0, 0)
    A = m.f12_from_flat_ints(a)
    B = None if b is None else m.f12_from_flat_ints(b)
    fl = m.f12_flat_ints
    return {
        "tower:fp2_mul": lambda: pad(m.f2_mul(f2(a), f2(b))), "tower:fp2_sqr": lambda: pad(m.f2_sqr(f2(a))),
        "tower:fp6_mul": lambda: pad(_flat6(m.f6_mul(f6(a), f6(b)))), "tower:fp6_sqr": lambda: pad(_flat6(m.f6_mul(f6(a), f6(a)))),
        "tower:fp12_mul": lambda: fl(m.f12_mul(A, B)), "tower:fp12_sqr": lambda: fl(m.f12_sqr(A)),
        "tower:fp12_014": lambda: fl(m.f12_mul(A, m._sparse_014(f2(b), (b[2], b[3]), (b[4], b[5])))),
        "tower:fp12_frob": lambda: fl(m.f12_frob(A)), "tower:fp12_conj": lambda: fl(m.f12_conj(A)),
        "tower2:fp2_nr": lambda: pad(m.f2_mul_xi(f2(a))), "tower2:fp2_mulfp": lambda: pad([a[0] * b[0] % P, a[1] * b[0] % P]),
        "tower2:fp6_by1": lambda: pad(_flat6(m.f6_mul(f6(a), (z, f2(b), z)))),
        "tower2:fp6_by01": lambda: pad(_flat6(m.f6_mul(f6(a), (f2(b), (b[2], b[3]), z)))),
        "tower2:fp6_nr": lambda: pad(_flat6(m.f6_mul_by_v(f6(a)))),
        "inv:fp2": lambda: pad(m.f2_inv(f2(a))) if any(a[:2]) else [0] * 12,
        "inv:fp6": lambda: pad(_flat6(m.f6_inv(f6(a)))) if any(a[:6]) else [0] * 12,
        "inv:fp12": lambda: fl(m.f12_inv(A)) if any(a) else [0] * 12,
    }[name]()


def _ksq_model(a, nsq):
    """nsq compressed squarings of the (z2 .. z5) of record a with Python integers (Karabina's formulas in this tower's coordinates):
    -> {number of squarings: (z2, z3, z4, z5)}"""
    sc = lambda x, k: (x[0] * k % P, x[1] * k % P)
    z = {2: (a[6], a[7]), 3: (a[4], a[5]), 4: (a[2], a[3]), 5: (a[10], a[11])}
    out = {}
    for e in range(1, nsq + 1):
        s45 = m.f2_add(m.f2_sqr(z[4]), m.f2_mul_xi(m.f2_sqr(z[5])))
        s23 = m.f2_add(m.f2_sqr(z[2]), m.f2_mul_xi(m.f2_sqr(z[3])))
        z = {2: m.f2_add(sc(m.f2_mul_xi(m.f2_mul(z[4], z[5])), 6), sc(z[2], 2)), 3: m.f2_sub(sc(s45, 3), sc(z[3], 2)),
             4: m.f2_sub(sc(s23, 3), sc(z[4], 2)), 5: m.f2_add(sc(m.f2_mul(z[2], z[3]), 6), sc(z[5], 2))}
        out[e] = (z[2], z[3], z[4], z[5])
    return out


def _check_stats(name, stats):
    mx = SEARCHED["maxima"][name]
    for t, v in stats.items():
        assert v < HARD[t], (name, t, v)
        assert v <= mx.get(t, 0), "%s: %s reached %r, above the %r recorded in adversarial_operands.json - headroom was eaten or the JSON is stale" % (name, t, v, mx.get(t, 0))


@pytest.mark.parametrize("name", [n for n in gen.programs() if n.startswith(("tower", "inv")) and n != "tower:cyc_sqr"])
def test_tower_programs_on_the_pool_and_the_searched_vectors(name):
    """every tower program of both tables and the three inversions (program A / inverse / program B; zero inputs among the records):
    the big-integer model's value, no emulator assertion, columns inside the int64, nothing above the recorded maxima"""
    def check(label, a, b, res):
        assert res == _model(name, a, b), (name, label)

    _replay(name, check)


def _searched(name):
    return [(v["label"], [H(x) for x in v["a"]], [H(x) for x in v["b"]] if v.get("b") else None) for v in SEARCHED["vectors"] if v["program"] == name]


def _replay(name, check):
    """pool records and searched vectors of a program through the emulator with the statistics on; check(label, a, b, result).  The
    headroom is judged first: a program that accumulates more than it should is named as that, not as a wrong value"""
    wa, wb = gen.programs()[name]
    results = []
    cg.STATS = {}
    try:
        for label, a, b in gen.start_records(name, wa, wb) + _searched(name):
            results.append((label, a, b, gen.run_program(name, a, b)))
        stats = dict(cg.STATS)
    finally:
        cg.STATS = None
    _check_stats(name, stats)
    for label, a, b, res in results:
        check(label, a, b, res)


def test_cyclotomic_squaring_program_on_adversarial_records():
    """cyc_sqr on cyclotomic images of adversarial records against the model, and on ARBITRARY records for the assertions and the
    recorded maxima (the formulas need no group element)"""
    for nm, a in adv.records(12, n_drawn=8)[::8]:
        if any(a):
            f = m.f12_from_flat_ints(a)
            g = m.f12_mul(m.f12_conj(f), m.f12_inv(f))
            g = m.f12_mul(m.f12_frob(m.f12_frob(g)), g)
            assert gen.run_program("tower:cyc_sqr", m.f12_flat_ints(g)) == m.f12_flat_ints(m.f12_sqr(g)), nm
    _replay("tower:cyc_sqr", lambda label, a, b, res: None)


@pytest.mark.parametrize("name", ["ksq"] + sorted(gen.KSQ_LONG))
def test_compressed_squaring_runs_on_arbitrary_records(name):
    """emu_ksq on arbitrary (not group) records - 3 squarings on every pool record, 1 / 17 / 48 / 63 squarings with several snapshot
    masks on every fortieth - against Karabina's closed formulas; nothing above the recorded maxima"""
    nsq, mask = gen.ksq_params(name)

    def check(label, a, b, res):
        want = _ksq_model(a, nsq)
        got = [((v[6], v[7]), (v[4], v[5]), (v[2], v[3]), (v[10], v[11])) for v in res]
        assert got == [want[e + 1] for e in range(nsq) if (mask >> e) & 1], (name, label)

    _replay(name, check)


@pytest.mark.parametrize("name", sorted(gen.KDEC_BRANCH))
def test_decompression_kernels_in_all_three_branches(name):
    """k_kdec_a / k_kdec_b (with the batched inversion's value between them) on adversarial (z2 .. z5): the regular branch, z2 == 0
    and z2 == z3 == 0, against the closed formulas; nothing above the recorded maxima"""
    def check(label, a, b, res):
        r = gen.kdec_record(name, a)
        z0, z1 = _decompress_model((r[6], r[7]), (r[4], r[5]), (r[2], r[3]), (r[10], r[11]))
        want = list(r)
        want[0], want[1], want[8], want[9] = z0[0], z0[1], z1[0], z1[1]
        assert res == want, (name, label)

    _replay(name, check)


def test_mulacc_block_on_adversarial_and_searched_operands():
    """the hand-scheduled MULACC block (tools/coopasm.py, executed by tools/asmemu.py) against the emulator's reduced columns, as
    tests/test_coopasm.py checks it on one random operand set - here on extreme stored digits and on the searched vectors"""
    recs = dict(adv.records(12))
    pick = [k for k in recs if "balanced-digits" in k and k.startswith("uniform")][:2] + [k for k in recs if k.startswith("alternating")][:1]
    for op in ("fp12_mul", "fp12_sqr", "fp12_014", "cyc_sqr", "fp6_mul"):
        cases = [(recs[k], recs[pick[(i + 1) % len(pick)]]) for i, k in enumerate(pick)]
        cases += [([H(x) for x in v["a"]], [H(x) for x in v["b"]] if v.get("b") else [H(x) for x in v["a"]]) for v in SEARCHED["vectors"] if v["program"] == "tower:" + op][:2]
        for a, b in cases:
            em = cg.Emu(wire_in=a, wire_in2=b)
            assert _check_program(cg.prog_tower(op), cg.LDS_SLOTS, cg.N_CONST, em) >= 1, op


# ---- the division-step inversion -----------------------------------------------------------------------------------------------
def _edge_words():
    w = [0, 1, (1 << 30) - 1, 1 << 29, 0x2AAAAAAA, 0x15555555, 0x3FFFFFFE, 0x20000001] + [1 << k for k in range(1, 30)]
    return w


def test_packed_division_steps_equal_the_plain_ones():
    """divsteps30_packed (the kernel's formulation: 16-bit halves, three runs, 24-bit multiplies; it asserts its own ranges) gives
    the matrix and the eta of thirty plain steps: on every (eta, f, g) the inversion meets on the pool and the searched values, on
    structured low words, for every eta from -31 to 31, and on a seeded random sample"""
    seen = set()
    vals = [op.v for op in adv.pool()] + [H(d["g"]) for d in SEARCHED["divsteps"]]
    for x in vals:                                           # the whole pool, every pre-image included
        tr = {}
        assert sgm.inv(x, trace=tr) == (pow(x, -1, P) if x else 0)
        seen.update(tr["lows"])
    for eta, f0, g0 in seen:
        assert sgm.divsteps30_packed(eta, f0, g0) == sgm.divsteps30(eta, f0, g0), (eta, f0, g0)
    fs = [w | 1 for w in _edge_words()]
    for f0 in fs:
        for g0 in _edge_words():
            for eta in (-1, -2, 0, 1, -31, 31):
                assert sgm.divsteps30_packed(eta, f0, g0) == sgm.divsteps30(eta, f0, g0), (eta, f0, g0)
    for eta in range(-31, 32):
        for f0 in fs[:12]:
            for g0 in (0, 1, 1 << 29, (1 << 30) - 1, 0x2AAAAAAA, 0x15555555):
                assert sgm.divsteps30_packed(eta, f0, g0) == sgm.divsteps30(eta, f0, g0), (eta, f0, g0)
    g = adv._Rng(0xD1)
    for _ in range(2000):
        eta, f0, g0 = g.below(63) - 31, g.below(1 << 30) | 1, g.below(1 << 30)
        assert sgm.divsteps30_packed(eta, f0, g0) == sgm.divsteps30(eta, f0, g0), (eta, f0, g0)
    # a g with thirty trailing zero bits: the batch matrix is ((2^30, 0), (0, 1)) - an entry of exactly 2^30
    assert sgm.divsteps30_packed(-1, sgm.PL[0], 0)[1] == (1 << 30, 0, 0, 1)


def test_packed_inversion_on_the_whole_pool():
    """inv() through the packed model equals pow(x, -1, p) on the whole pool (pre-images included) and on the searched values; the
    batches needed and the extremes of d, e and the matrix entries stay within what the JSON records, and inside 37 batches"""
    mx = SEARCHED["maxima"]["divsteps"]
    worst = {}
    for op in adv.pool() + [adv.Op("searched", d["label"], H(d["g"])) for d in SEARCHED["divsteps"]]:
        tr = {}
        assert sgm.inv(op.v, packed=True, trace=tr) == (pow(op.v, -1, P) if op.v else 0), op
        if op.v:
            for t, v in (("batches", tr["batches"]), ("de_hi", tr["de_hi"]), ("de_lo", -tr["de_lo"]), ("run_max", tr["run_max"]), ("entry_max", tr["entry_max"])):
                worst[t] = max(worst.get(t, 0), v)
    assert worst == mx, (worst, mx)
    assert worst["batches"] <= sgm.NB and worst["run_max"] <= 1 << 10 and worst["entry_max"] <= 1 << 30 and worst["de_hi"] <= 1 and worst["de_lo"] < 2
    for d in SEARCHED["divsteps"]:
        tr = {}
        sgm.inv(H(d["g"]), packed=True, trace=tr)
        got = {"batches": tr["batches"], "de_hi": tr["de_hi"], "de_lo": -tr["de_lo"], "run_max": tr["run_max"], "entry_max": tr["entry_max"]}[d["target"]]
        assert got == d["value"], d["label"]
        assert sgm.NB - tr["batches"] >= sgm.NB - mx["batches"] > 0          # batches left over when g == 0 is reached


def test_committed_json_is_what_the_search_writes_for_its_header():
    hdr = SEARCHED["header"]
    assert (hdr["seed"], hdr["evals_per_climb"], hdr["evals_divstep"], hdr["ksq"]) == (gen.SEED, gen.EVALS_PER_CLIMB, gen.EVALS_DIVSTEP, [gen.KSQ_NSQ, gen.KSQ_MASK])
    assert SEARCHED["findings"] == []
    assert set(SEARCHED["maxima"]) == set(gen.programs()) | {"divsteps"}
    assert os.path.getsize(adv.JSON_PATH) < 256 * 1024
