"""Batches for zkp_kzg_cell_verify_batch built in EXPONENT space (helper of test_cell_verify_cpu.py and test_gpu_cell_verify.py; not a test
module).  A G1 point is [e] g1 for a known e, so a cell is (commitment exponent, index, values, proof exponent), its infinity flags follow
from exponent 0, and the verdict of ANY crafted batch - forgeries that only the right random scalars tell apart included - is known from
the combined equation on Python integers (cells_model.batch_holds) without the library under test.  The values come from the model's
transform of the zero-padded coefficients (cells_model.extended_values), never from Horner's rule per point.

The forgeries.  With r_j = a_j + b_j z^2 the verifier checks
    tau^l sum r_j pi_j = sum r_j C_j + sum r_j c_j^l pi_j - sum r_j I_j(tau).
Each forgery changes two cells so that THIS equation still holds under the batch's own scalars, and no longer under any other: it is
accepted exactly when every place of the device code that carries r_j carries the same a_j + b_j z^2."""
import random

import numpy as np

import bls12_381_model as bm
import cells_model as cm
import cells_replay_cases as crc
import poly_model as pm

R = pm.R
Z2 = bm.BLS_X ** 2                                   # the constant tests/test_rlc_cpu.py pins
TAU = crc.TAU


def scalar(ab):
    """r_j = a_j + b_j z^2 mod r"""
    return (int(ab[0]) + int(ab[1]) * Z2) % R


def pairs(rng, n):
    """n pairs (a, b) of 64-bit words from a seeded generator, a odd: no (0, 0)"""
    return [(rng.getrandbits(64) | 1, rng.getrandbits(64)) for _ in range(n)]


class Batch:
    """shape = (log2_n, log2_l, log2_ext, bitrev); cells = [(commitment exponent, index, values, proof exponent)]; rand = [(a, b)];
    invalid = [(where, position, wire point)] with where in c / proof / monomial / g2 / tau_l_g2: points outside the groups that wire()
    puts in and that want() refuses by construction"""

    def __init__(self, shape, cells, rand, tau=TAU, invalid=()):
        self.shape, self.tau = tuple(shape), tau
        self.cells = [(c % R, int(m), tuple(int(v) for v in vals), p % R) for c, m, vals, p in cells]
        self.rand = [(int(a), int(b)) for a, b in rand]
        self.invalid = list(invalid)
        assert len(self.cells) == len(self.rand)

    n = property(lambda self: len(self.cells))
    log2_l = property(lambda self: self.shape[1])
    log2_d = property(lambda self: self.shape[0] + self.shape[2])
    big_m = property(lambda self: 1 << (self.shape[0] + self.shape[2] - self.shape[1]))
    bitrev = property(lambda self: self.shape[3])

    def rs(self):
        return [scalar(ab) for ab in self.rand]

    def replace(self, cells=None, rand=None, invalid=None):
        return Batch(self.shape, self.cells if cells is None else cells, self.rand if rand is None else rand, self.tau,
                     self.invalid if invalid is None else invalid)

    def with_cell(self, j, c=None, m=None, values=None, p=None):
        cells = list(self.cells)
        old = cells[j]
        cells[j] = (old[0] if c is None else c, old[1] if m is None else m, old[2] if values is None else values, old[3] if p is None else p)
        return self.replace(cells=cells)

    def with_value(self, j, u, v):
        vals = list(self.cells[j][2])
        vals[u] = v
        return self.with_cell(j, values=vals)

    def with_rand(self, rand):
        return self.replace(rand=[(int(a), int(b)) for a, b in rand])

    def with_pair(self, j, a=None, b=None):
        rand = list(self.rand)
        rand[j] = (rand[j][0] if a is None else a, rand[j][1] if b is None else b)
        return self.replace(rand=rand)

    def with_invalid(self, where, pos, point):
        return self.replace(invalid=self.invalid + [(where, pos, point)])

    def take(self, idx):
        return self.replace(cells=[self.cells[j] for j in idx], rand=[self.rand[j] for j in idx])


# ------------------------------------------------------------------------------------------------------------------- valid batches
_polys = {}


def poly_data(f, shape, tau=TAU):
    """(commitment exponent, the M rows of l values, the M proof exponents) of polynomial f; the values through the model's transform"""
    log2_n, log2_l, log2_ext, bitrev = shape
    key = (tuple(f), shape, tau)
    if key not in _polys:
        _, l, _, _, big_m = cm.sizes(log2_n, log2_l, log2_ext)
        if bitrev:
            rows = cm.extended_values(f, log2_n, log2_l, log2_ext, True)
        else:                                        # natural order: cell m is ev[m + M u], u < l
            ev = [v for row in cm.extended_values(f, log2_n, log2_l, log2_ext, False) for v in row]
            rows = [[ev[m + big_m * u] for u in range(l)] for m in range(big_m)]
        _polys[key] = (cm.horner(f, tau), rows, cm.quotient_proofs(f, tau, log2_n, log2_l, log2_ext, bitrev))
    return _polys[key]


def batch_of(polys, picks, shape, seed, tau=TAU):
    """the cells picks = [(polynomial, cell index)] of the polynomials, with seeded scalars"""
    data = [poly_data(f, shape, tau) for f in polys]
    cells = [(data[j][0], m, data[j][1][m], data[j][2][m]) for j, m in picks]
    return Batch(shape, cells, pairs(random.Random(seed), len(picks)), tau)


def valid_batch(shape, n, seed, n_polys=2, tau=TAU):
    """n cells of n_polys random polynomials; every (polynomial, cell) pair appears before any repeats"""
    log2_n, log2_l, log2_ext, _ = shape
    rng = random.Random(seed)
    polys = [[rng.randrange(R) for _ in range(1 << log2_n)] for _ in range(n_polys)]
    big_m = 1 << (log2_n + log2_ext - log2_l)
    every = [(j, m) for j in range(n_polys) for m in range(big_m)]
    rng.shuffle(every)
    picks = [every[i] if i < len(every) else every[rng.randrange(len(every))] for i in range(n)]
    return batch_of(polys, picks, shape, seed + 1, tau)


def zero_polynomial(shape):
    return [0] * (1 << shape[0])


def low_degree_polynomial(shape, seed):
    """degree below l: its cells' interpolants are the polynomial itself, every quotient is zero"""
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(1 << shape[1])] + [0] * ((1 << shape[0]) - (1 << shape[1]))


# ------------------------------------------------------------------------------------------------------------------- the forgeries
def _inv(x):
    return pow(x, -1, R)


def shift_commitments(b, i, j, d, half=False):
    """C_i += d, C_j -= d: the plain sum of the commitments is unchanged.  Holds iff r_i = r_j"""
    assert i != j and d % R
    out = b.with_cell(i, c=b.cells[i][0] + d)
    return out if half else out.with_cell(j, c=b.cells[j][0] - d)


def weighted_commitments(b, i, j, d, half=False):
    """C_i += r_j d, C_j -= r_i d: holds iff the verifier's r is exactly a + b z^2"""
    assert i != j and d % R
    r = b.rs()
    out = b.with_cell(i, c=b.cells[i][0] + r[j] * d)
    return out if half else out.with_cell(j, c=b.cells[j][0] - r[i] * d)


def delta_interpolant_at_tau(b, i, u, delta):
    """(the Lagrange interpolant of delta e_u on cell i's points)(tau): one term of Lagrange's formula"""
    log2_n, log2_l, log2_ext, bitrev = b.shape
    pts = cm.cell_points(b.cells[i][1], log2_n, log2_l, log2_ext, bitrev)
    num = den = 1
    for t, q in enumerate(pts):
        if t != u:
            num, den = num * (b.tau - q) % R, den * (pts[u] - q) % R
    return delta * num % R * _inv(den) % R


def value_for_commitment(b, i, u, delta, j, half=False):
    """value u of cell i += delta, C_j += (r_i / r_j) dI_i(tau): holds iff the fold weighs cell i's interpolant with the MSM's r_i"""
    assert i != j and delta % R
    r = b.rs()
    out = b.with_value(i, u, (b.cells[i][2][u] + delta) % R)
    return out if half else out.with_cell(j, c=b.cells[j][0] + r[i] * _inv(r[j]) % R * delta_interpolant_at_tau(b, i, u, delta))


def proof_for_commitment(b, i, d, j, half=False):
    """pi_i += d, C_j += (r_i / r_j) d (tau^l - c_i^l): holds iff ms[n + i] = r_i c_i^l and row 1 carries r_i"""
    assert i != j and d % R
    log2_n, log2_l, log2_ext, bitrev = b.shape
    l = 1 << log2_l
    r = b.rs()
    c_l = pow(cm.coset_shift(b.cells[i][1], log2_n, log2_l, log2_ext, bitrev), l, R)
    out = b.with_cell(i, p=b.cells[i][3] + d)
    return out if half else out.with_cell(j, c=b.cells[j][0] + r[i] * _inv(r[j]) % R * d % R * (pow(b.tau, l, R) - c_l))


def forgeries(b, i, j, us, rng):
    """(name, crafted batch, its half-applied version) of every forgery on cells i and j; us: the value positions"""
    d = rng.randrange(1, R)
    out = [("weighted_commitments", weighted_commitments(b, i, j, d), weighted_commitments(b, i, j, d, half=True)),
           ("proof_for_commitment", proof_for_commitment(b, i, d, j), proof_for_commitment(b, i, d, j, half=True))]
    for u in us:
        out.append(("value_for_commitment-u%d" % u, value_for_commitment(b, i, u, d, j), value_for_commitment(b, i, u, d, j, half=True)))
    return out


# ------------------------------------------------------------------------------------------------------------------- the verdict
def holds(b):
    """the combined equation on exponents under the batch's own scalars (values and indices taken as they are: callers rule out the
    non-canonical ones first)"""
    log2_n, log2_l, log2_ext, bitrev = b.shape
    return cm.batch_holds(b.cells, b.rs(), b.tau, log2_n, log2_l, log2_ext, bitrev)


def facts(b):
    """what holds by construction: every value < r, every index < M, no (0, 0) pair, no invalid point"""
    return (all(v < R for _, _, vals, _ in b.cells for v in vals) and all(m < b.big_m for _, m, _, _ in b.cells)
            and all(a or bb for a, bb in b.rand) and not b.invalid)


def want(b):
    return facts(b) and holds(b)


def want_each(b):
    """cell by cell, by the definition (Lagrange's formula): what kzg_cell_verify_each must answer"""
    log2_n, log2_l, log2_ext, bitrev = b.shape
    return [all(v < R for v in vals) and m < b.big_m and cm.cell_holds(c, m, vals, p, b.tau, log2_n, log2_l, log2_ext, bitrev) for c, m, vals, p in b.cells]


# ------------------------------------------------------------------------------------------------------------------- the wire
_points = {}
_monomials = {}


def points_of(exps):
    """[e] g1 by the oracle, each distinct exponent once per process"""
    import replay_cases as rc
    exps = [e % R for e in exps]
    new = sorted({e for e in exps if e not in _points})
    if new:
        pts, _ = rc.expect_points(1, new)
        for e, p in zip(new, pts):
            _points[e] = p
    return np.stack([_points[e] for e in exps]), np.array([1 if e == 0 else 0 for e in exps], dtype=np.uint8)


def monomial_points(h, log2_l, tau=TAU):
    """[tau^i] g1, i < l: by the oracle up to 2^8 points, beyond by the helper engine's g1_mul (the GPU test holds entries of it to the oracle)"""
    import replay_cases as rc
    key = (log2_l, tau)
    if key not in _monomials:
        if log2_l <= 8:
            _monomials[key] = crc.monomial_for(log2_l, tau)
        else:
            _monomials[key] = rc._g1(h, [pow(tau, i, R) for i in range(1 << log2_l)])
    return _monomials[key]


def wire(b, h=None):
    """the arrays of engine.kzg_cell_verify, by name; with the helper engine h also the verifier's setup (monomial, g2, tau_l_g2)"""
    import replay_cases as rc
    c, inf_c = points_of([x[0] for x in b.cells])
    p, inf_p = points_of([x[3] for x in b.cells])
    t = dict(c=c.copy(), inf_c=inf_c, index=np.array([x[1] for x in b.cells], dtype=np.uint32), proof=p.copy(), inf_proof=inf_p,
             values=rc.fr_rows([v for x in b.cells for v in x[2]]), rand=np.array(b.rand, dtype=np.uint64).reshape(b.n, 2))
    if h is not None:
        t.update(monomial=monomial_points(h, b.log2_l, b.tau).copy(), g2=crc.g2_generator(), tau_l_g2=crc.tau_l_g2_for(h, b.log2_l, b.tau).copy())
    for where, pos, point in b.invalid:
        if where in ("g2", "tau_l_g2"):
            t[where] = np.asarray(point, dtype=np.uint64).copy()
        else:
            t[where][pos] = point
    return t


# ------------------------------------------------------------------------------------------------------------------- invalid points the equation cannot see
# A point outside the groups in place of a valid one also breaks the equation, so its verdict says nothing about the status bytes.  These do
# not: (1) P + T for a valid P and a T of small order h on the curve, under a scalar r_j that h divides - [r_j](P + T) = [r_j] P, so the
# MSM's sums are what they were (for a proof: in a cell of index 0, where r_j c_j^l = r_j); (2) any point at all in a monomial position
# whose scalar -a_i is zero because coefficient i of every cell's interpolant is.  Only the points check can refuse them.
def pairs_divisible_by(rng, n, h):
    """n pairs (a, b), a non-zero, with a + b z^2 (below 2^192, so not reduced) divisible by h"""
    out = []
    for _ in range(n):
        a, b = rng.getrandbits(62) | 1, rng.getrandbits(64)
        a += -(a + b * Z2) % h
        assert 0 < a < 1 << 64 and (a + b * Z2) % h == 0 and a + b * Z2 < R
        out.append((a, b))
    return out


def plus_small_order(point, torsion):
    """the wire point P + T on Python integers (bls12_381_model): on the curve, outside the subgroup"""
    import outside_groups as og
    import replay_cases as rc
    q = bm.g1_add((rc._fe(point, 0), rc._fe(point, 1)), torsion)
    assert q is not None and bm.g1_on_curve(q) and not bm.g1_torsion_free(q)
    return og.g1_wire(q)


def sparse_low_degree_polynomial(shape, seed, keep):
    """degree below l with only the coefficients in `keep` non-zero: coefficient i of every interpolant is f_i, zero elsewhere"""
    rng = random.Random(seed)
    return [rng.randrange(1, R) if i in keep else 0 for i in range(1 << shape[1])] + [0] * ((1 << shape[0]) - (1 << shape[1]))


# ------------------------------------------------------------------------------------------------------------------- the GPU tests' shapes
# (log2_d, log2_l, n); N = D / 2, but N = D where M = 1.  test_cell_verify_cpu.py holds each to the planners' own arithmetic
GPU_SHAPES = {
    "S-parts": (7, 2, 130),        # l = 4: rows = 64, three parts of the fold, the last of 2 rows
    "S-one": (5, 0, 300),          # l = 1: rows = 256, two parts; 64 distinct cells, so repeats are certain
    "S-tiles": (9, 7, 9),          # l = 128: two tiles of the fold, rows = 4, three parts
    "S-big": (13, 11, 6),          # l = 2048: above one tile of the transform, 32 tiles of the fold
    "S-m1-l8": (3, 3, 2),          # M = 1
    "S-m1-l1": (0, 0, 1),
    "S-inf": (7, 2, 5),            # the shapes of the infinities, of the points outside the groups and of the mixed batches
    "S-outside": (7, 2, 3),
    "S-mixed-l16": (6, 4, 20),
}


def model_shape(name, bitrev):
    log2_d, log2_l, _ = GPU_SHAPES[name]
    ext = 0 if log2_l == log2_d else 1
    return (log2_d - ext, log2_l, ext, bool(bitrev))


def gpu_batch(name, bitrev, n=None):
    """the valid batch of a named shape; one per (name, order, n) and process"""
    n = GPU_SHAPES[name][2] if n is None else n
    key = (name, bool(bitrev), n)
    if key not in _batches:
        _batches[key] = valid_batch(model_shape(name, bitrev), n, 0xCE11 + 97 * sorted(GPU_SHAPES).index(name) + bool(bitrev))
    return _batches[key]


_batches = {}
