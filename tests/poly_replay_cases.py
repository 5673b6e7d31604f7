"""The capturable device-pointer entry points of include/zkp_poly.h (helper of test_gpu_poly_replay.py, test_gpu_kzg_open.py and
test_poly_cpu.py; not a test module): Case rows in the form of tests/replay_cases.py, and the KZG producer fixtures the opening tests
share.  Expected values never come from the library under test: field values are Python integers (tests/poly_model.py, Horner), and
every point is [e] g1 for an exponent e known from the construction - the setup is built from a known tau, so a commitment is
[f(tau)] g1 and a proof [(f(tau) - y) / (tau - z)] g1 - which is one oracle multiplication of the generator (replay_cases.expect_points).
The setup points themselves are inputs, made through a second engine that never captures."""
import random

import numpy as np

import poly_model as pm
import replay_cases as rc
from replay_cases import Case, fr_rows

R = pm.R

# every zkp_*_dev( of include/zkp_poly.h has a row below or a written reason here
EXCLUDED = {}


# ------------------------------------------------------------------------------------------------------------------- the NTT
def ntt_sets(log2_n, n_poly, flags, seed):
    """three sets of n_poly polynomials: random / the adversarial ends of the field / sparse"""
    def build():
        rng = random.Random(seed * 977 + log2_n * 31 + n_poly * 7 + flags)
        n = 1 << log2_n
        sets, exp = [], []
        for s in range(3):
            if s == 0:
                polys = [[rng.randrange(R) for _ in range(n)] for _ in range(n_poly)]
            elif s == 1:
                polys = [[(R - 1, 0, 1, R - 2)[(i + j) % 4] for i in range(n)] for j in range(n_poly)]
            else:
                polys = [[rng.randrange(R) if i in (0, 1, n // 2 + 1, n - 1) else 0 for i in range(n)] for _ in range(n_poly)]
            sets.append(dict(x=fr_rows([v for p in polys for v in p])))
            exp.append((fr_rows([v for p in polys for v in pm.ntt_flags(p, log2_n, flags)]),))
        return sets, exp
    return rc._cached(("ntt", log2_n, n_poly, flags, seed), build)


def _ntt_run(e, t, sh):
    return (e.fr_ntt(t["x"], sh[1], inverse=bool(sh[2] & pm.INVERSE), bitrev=bool(sh[2] & pm.BITREV), coset=bool(sh[2] & pm.COSET)),)


# ------------------------------------------------------------------------------------------------------------------- the KZG producer
TAU = 0x5EED0000000000000000000000000000000000000000000000000000C0FFEE % R


class Setup:
    """the Lagrange setup of the 2^log2_n-point domain for the known TAU, in the order of the evaluations (bit-reversed with bitrev)"""

    def __init__(self, h, log2_n, bitrev):
        self.log2_n, self.bitrev, self.n = log2_n, bitrev, 1 << log2_n
        n = self.n
        dom = pm.domain(log2_n)
        self.slot_domain = [dom[pm.bit_reverse(i, log2_n) if bitrev else i] for i in range(n)]          # the domain point of slot i
        assert all(TAU != d for d in dom)
        scale = (pow(TAU, n, R) - 1) * pow(n, -1, R) % R
        self.lagrange_tau = [scale * d % R * pow(TAU - d, -1, R) % R for d in self.slot_domain]           # l_i(tau)
        assert sum(self.lagrange_tau) % R == 1
        self.lagrange_g1 = rc._g1(h, self.lagrange_tau)
        assert all(self.lagrange_tau)


def setup_for(h, log2_n, bitrev):
    return rc._cached(("kzg-setup", log2_n, bitrev), lambda: Setup(h, log2_n, bitrev))


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


POLY_KINDS = ("random", "zero", "constant", "top")       # "top": a polynomial of degree N - 1
Z_KINDS = ("outside", "zero", "slot0", "slot1", "slotlast")


def make_poly(kind, n, rng):
    if kind == "zero":
        return [0] * n
    if kind == "constant":
        return [rng.randrange(1, R)] + [0] * (n - 1)
    if kind == "top":
        return [0] * (n - 1) + [rng.randrange(1, R)] if n > 1 else [rng.randrange(1, R)]
    return [rng.randrange(R) for _ in range(n)]


def make_z(kind, setup, rng):
    if kind == "zero":
        return 0
    if kind.startswith("slot"):
        m = {"slot0": 0, "slot1": min(1, setup.n - 1), "slotlast": setup.n - 1}[kind]
        return setup.slot_domain[m]
    while True:
        z = rng.randrange(R)
        if pow(z, setup.n, R) != 1:
            return z


def opening(setup, polys, zs):
    """coefficient lists and points -> the call's inputs (evals, z) and everything expected of it, from Python integers and the oracle"""
    evals = [pm.ntt(c, setup.log2_n, bitrev=setup.bitrev) for c in polys]
    f_tau = [horner(c, TAU) for c in polys]
    y = [horner(c, z) for c, z in zip(polys, zs)]
    q_tau = [(ft - yy) * pow(TAU - z, -1, R) % R for ft, yy, z in zip(f_tau, y, zs)]
    proof, inf = rc.expect_points(1, q_tau)
    commit, cinf = rc.expect_points(1, f_tau)
    return dict(evals=fr_rows([v for e in evals for v in e]), z=fr_rows(zs), y=fr_rows(y), proof=proof, inf=inf, commit=commit, cinf=cinf)


def open_sets(h, n, log2_n, bitrev, seed):
    """three sets of n polynomials of one setup: A random polynomials at points outside the domain; B the four kinds of polynomial with
    z in the domain at different slots, at zero and outside; C random polynomials, all in the domain"""
    def build():
        rng = random.Random(seed * 131 + n * 17 + log2_n * 3 + bitrev)
        st = setup_for(h, log2_n, bitrev)
        big_n = st.n
        sets, exp = [], []
        for s in range(3):
            if s == 0:
                polys = [make_poly("random", big_n, rng) for _ in range(n)]
                zs = [make_z("outside", st, rng) for _ in range(n)]
            elif s == 1:
                polys = [make_poly(POLY_KINDS[j % 4], big_n, rng) for j in range(n)]
                zs = [make_z(("slot1", "slotlast", "zero", "outside", "slot0")[j % 5], st, rng) for j in range(n)]
            else:
                polys = [make_poly("random", big_n, rng) for _ in range(n)]
                zs = [st.slot_domain[rng.randrange(big_n)] for _ in range(n)]
            d = opening(st, polys, zs)
            sets.append(dict(lagrange=st.lagrange_g1, evals=d["evals"], z=d["z"]))
            exp.append((d["y"], d["proof"], d["inf"]))
        return sets, exp
    return rc._cached(("kzg-open", n, log2_n, bitrev, seed), build)


CASES = [
    Case("fr_ntt-log12-x5-flags%d" % flags, ["zkp_fr_ntt_batch_dev"], "fr_ntt", lambda h, shape, seed: ntt_sets(shape[1], shape[0], shape[2], seed), _ntt_run,
         (5, 12, flags), (2, 4, flags)) for flags in (0, pm.BITREV | pm.COSET, pm.INVERSE | pm.BITREV, pm.INVERSE | pm.COSET)
] + [
    Case("kzg_open-n3-N256%s" % ("-bitrev" if br else ""), ["zkp_kzg_open_batch_dev"], "kzg_open",
         lambda h, shape, seed: open_sets(h, shape[0], shape[1], shape[2], seed),
         lambda e, t, sh: e.kzg_open(t["lagrange"], t["evals"], t["z"], sh[1], sh[2]), (3, 8, br), (1, 2, br), "memset/copy") for br in (False, True)
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
