"""The capturable device-pointer entry points of include/zkp_cells.h (helper of test_gpu_cells_replay.py, test_gpu_cells.py,
test_gpu_call_order_cells.py and test_cells_cpu.py; not a test module): Case rows in the form of tests/replay_cases.py, and the fixtures the
cell tests share.  Expected values never come from the library under test: every point is [e] g1 for an exponent e known from the
DEFINITION of a cell proof (tests/cells_model.py: the quotient by X^l - c^l on Python integers, the TAU of tests/poly_replay_cases.py), which
is one oracle multiplication of the generator (replay_cases.expect_points); every verdict is known from how the cells were made."""
import random

import numpy as np

import cells_model as cm
import fk20_replay_cases as frc
import poly_model as pm
import poly_replay_cases as prc
import replay_cases as rc
from fk20_replay_cases import Lazy
from replay_cases import Case, fr_rows

R = pm.R
TAU = prc.TAU

# every zkp_*_dev( of include/zkp_cells.h has a row below or a written reason here
EXCLUDED = {}

POLY_KINDS = frc.POLY_KINDS
monomial_for = frc.monomial_for
make_poly = frc.make_poly


def cells_setup_for(log2_n, log2_l, tau=TAU):
    """(points, inf) expected of zkp_kzg_cells_setup, by the oracle"""
    return rc._cached(("cells-setup", log2_n, log2_l, tau), lambda: rc.expect_points(1, [e for v in cm.cells_setup(tau, log2_n, log2_l) for e in v]))


def proofs_for(polys, log2_n, log2_l, log2_ext, bitrev, tau=TAU):
    return rc.expect_points(1, [e for f in polys for e in cm.quotient_proofs(f, tau, log2_n, log2_l, log2_ext, bitrev)])


def tau_l_g2_for(h, log2_l, tau=TAU):
    return rc._cached(("cells-tau-l-g2", log2_l, tau), lambda: rc._g2(h, [pow(tau, 1 << log2_l, R)])[0])


def g2_generator():
    from zkvm_pairings_amd import synthetic
    return synthetic.G2_GENERATOR.copy()


def cell_rows(polys, picks, log2_n, log2_l, log2_ext, bitrev, tau=TAU):
    """the verifier's arrays for the cells picks = [(polynomial, cell index)], all from the definition: commitments, indices (int32: what a
    resident tensor holds), values, proofs with their flags"""
    vals = {j: cm.cell_values(polys[j], log2_n, log2_l, log2_ext, bitrev) for j in {j for j, _ in picks}}
    prf = {j: cm.quotient_proofs(polys[j], tau, log2_n, log2_l, log2_ext, bitrev) for j in vals}
    c, inf_c = rc.expect_points(1, [cm.horner(polys[j], tau) for j, _ in picks])
    p, inf_p = rc.expect_points(1, [prf[j][m] for j, m in picks])
    return dict(c=c, inf_c=inf_c, index=np.array([m for _, m in picks], dtype=np.int32), values=fr_rows([v for j, m in picks for v in vals[j][m]]),
                proof=p, inf_proof=inf_p)


# ---- one call across a slice boundary, assembled as slice_pools.fk20_call is: a pool of 11 polynomials with known proofs, a seeded index
# sequence over it, the short last slice made of pool items used nowhere else in the call
SLICE_LOG2, SLICE_LOG2_L, SLICE_EXT = 2, 1, 1
SLICE_LEN = (1 << 17) >> SLICE_LOG2               # floor(2^17 / N) polynomials: test_cells_cpu.py holds it to the planner's
SLICE_N = SLICE_LEN + 3
SLICE_B, SLICE_TAIL = 11, (7, 9, 10)


def slice_call(bitrev):
    import slice_pools as sp

    def build():
        rng = random.Random(sp.SEED * 9 + bitrev)
        polys = [make_poly(k, 1 << SLICE_LOG2, rng) for k in sp.fk20_kinds()]
        sp._distinct(polys)
        proof, inf = proofs_for(polys, SLICE_LOG2, SLICE_LOG2_L, SLICE_EXT, bitrev)
        return dict(polys=polys, coeffs=fr_rows([v for f in polys for v in f]), proof=proof, inf=inf)
    p = rc._cached(("slice-cells-pool", bitrev), build)
    idx = sp.draw(sp.SEED + 401 + bitrev, SLICE_N, SLICE_TAIL, SLICE_B)
    per_in, per_out = 1 << SLICE_LOG2, 1 << (SLICE_LOG2 - SLICE_LOG2_L + SLICE_EXT)
    return sp.Call(SLICE_N, SLICE_LEN, idx, dict(coeffs=(sp.take(p["coeffs"], SLICE_B, idx), per_in)),
                   dict(proof=(sp.take(p["proof"], SLICE_B, idx), per_out), inf=(sp.take(p["inf"], SLICE_B, idx), per_out)), p)


# ---- polynomials that make the additions of k_cell_mac and k_cell_sum meet +-X and +-partial under a setup with tau = 1 or tau = -1
# (cells_shapes.EXCEPTIONAL_SHAPES; cells_model.addition_cases counts the cases on exponents)
EXCEPTIONAL_TAUS = (1, R - 1)
EXCEPTIONAL_KINDS = ("equal", "blocks", "random", "zero", "equal", "minus-equal", "random")


def exceptional_polys(log2_n, log2_l, s, seed):
    """equal: every coefficient the same, so the l scalars of a slot are; blocks: the sign changes from one group of g = 2^s strides to the
    next (stride i sees the coefficients j = l - 1 - i mod l), so consecutive partials are opposite where the bases are equal"""
    rng = random.Random(seed)
    n, l = 1 << log2_n, 1 << log2_l
    out = []
    for kind in EXCEPTIONAL_KINDS:
        v = rng.randrange(1, R)
        if kind == "blocks":
            out.append([v if (((l - 1 - j % l) >> s) & 1) == 0 else R - v for j in range(n)])
        elif kind == "equal":
            out.append([v] * n)
        elif kind == "minus-equal":
            out.append([R - out[0][0]] * n)
        elif kind == "zero":
            out.append([0] * n)
        else:
            out.append([rng.randrange(1, R) for _ in range(n)])
    return out


def _setup_sets(log2_n, log2_l, seed):
    def build():
        rng = random.Random(seed * 59 + 7 * log2_n + log2_l)
        taus = [TAU if s == 0 else rng.randrange(2, R) for s in range(3)]
        return (Lazy([(lambda t: lambda: dict(monomial=monomial_for(log2_n, t)))(t) for t in taus]),
                Lazy([(lambda t: lambda: cells_setup_for(log2_n, log2_l, t))(t) for t in taus]))
    return rc._cached(("cells-setup-sets", log2_n, log2_l, seed), build)


def _cells_sets(n, log2_n, log2_l, log2_ext, bitrev, seed):
    def build():
        rng = random.Random(seed * 223 + n * 13 + log2_n * 3 + log2_l * 5 + log2_ext + bitrev)
        big_n = 1 << log2_n
        polys = [[make_poly(POLY_KINDS[(2 * s + j) % 5] if s else "random", big_n, rng) for j in range(n)] for s in range(3)]

        def inputs(f):
            setup, sinf = cells_setup_for(log2_n, log2_l)
            return dict(setup=setup, setup_inf=sinf, coeffs=fr_rows([v for p in f for v in p]))
        return (Lazy([(lambda f: lambda: inputs(f))(f) for f in polys]),
                Lazy([(lambda f: lambda: proofs_for(f, log2_n, log2_l, log2_ext, bitrev))(f) for f in polys]))
    return rc._cached(("cells-sets", n, log2_n, log2_l, log2_ext, bitrev, seed), build)


def _verify_sets(h, n, log2_n, log2_l, log2_ext, bitrev, seed):
    """A: every cell holds; B: the last cell carries the values of another cell; C: the first cell's proof is its commitment"""
    def build():
        rng = random.Random(seed * 227 + n * 17 + log2_n + log2_l)
        big_m = 1 << (log2_n - log2_l + log2_ext)
        polys = [make_poly("random", 1 << log2_n, rng) for _ in range(2)]
        sets, exp = [], []
        for s in range(3):
            picks = [(rng.randrange(2), rng.randrange(big_m)) for _ in range(n)]
            t = cell_rows(polys, picks, log2_n, log2_l, log2_ext, bitrev)
            if s == 1:
                other = cell_rows(polys, [(picks[-1][0], (picks[-1][1] + 1) % big_m)], log2_n, log2_l, log2_ext, bitrev)
                t["values"][-(1 << log2_l):] = other["values"]
            if s == 2:
                t["proof"][0], t["inf_proof"][0] = t["c"][0], t["inf_c"][0]
            t.update(monomial=monomial_for(log2_l), g2=g2_generator(), tau_l_g2=tau_l_g2_for(h, log2_l), rand=rc._ab(random.Random(seed + 8 + s), n))
            sets.append(t)
            exp.append((rc._i32(s == 0 or (s == 1 and big_m == 1)),))
        return sets, exp
    return rc._cached(("cells-verify-sets", n, log2_n, log2_l, log2_ext, bitrev, seed), build)


def verify_call(e, t, log2_d, log2_l, bitrev):
    return e.kzg_cell_verify(t["monomial"], t["g2"], t["tau_l_g2"], t["c"], t["index"], t["values"], t["proof"], log2_d, log2_l, bitrev=bitrev, inf_c=t["inf_c"],
                             inf_proof=t["inf_proof"], rand=t["rand"])


# shapes: setup (log2_n, log2_l); producer (n, log2_n, log2_l, log2_ext, bitrev); verifier (n, log2_n, log2_l, log2_ext, bitrev)
CASES = [
    Case("kzg_cells_setup-N64-l4", ["zkp_kzg_cells_setup_dev"], "kzg_cells_setup", lambda h, shape, seed: _setup_sets(shape[0], shape[1], seed),
         lambda e, t, sh: e.kzg_cells_setup(t["monomial"], sh[0], sh[1]), (6, 2), (2, 1)),
    Case("kzg_cells-n3-N64-l4-e2-bitrev", ["zkp_kzg_cells_batch_dev"], "kzg_cells", lambda h, shape, seed: _cells_sets(*shape, seed),
         lambda e, t, sh: e.kzg_cells(t["setup"], t["setup_inf"], t["coeffs"], sh[1], sh[2], sh[3], sh[4]), (3, 6, 2, 1, True), (1, 2, 1, 1, True)),
    Case("kzg_cell_verify-n5-N16-l4", ["zkp_kzg_cell_verify_batch_dev"], "kzg_cell_verify", lambda h, shape, seed: _verify_sets(h, *shape, seed),
         lambda e, t, sh: (verify_call(e, t, sh[1] + sh[3], sh[2], sh[4]),), (5, 4, 2, 1, True), (2, 2, 1, 1, True), "memset/copy"),
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
