"""The capturable device-pointer entry points of include/zkp_fk20.h (helper of test_gpu_fk20_replay.py, test_gpu_g1_ntt.py, test_gpu_fk20.py
and test_fk20_cpu.py; not a test module): Case rows in the form of tests/replay_cases.py, and the fixtures the FK20 tests share.  Expected
values never come from the library under test: every point is [e] g1 for an exponent e known from the construction (tests/fk20_model.py on
Python integers, the TAU of tests/poly_replay_cases.py), which is one oracle multiplication of the generator (replay_cases.expect_points)."""
import operator
import random

import numpy as np

import fk20_model as fm
import poly_model as pm
import poly_replay_cases as prc
import replay_cases as rc
from replay_cases import Case, fr_rows

R = pm.R
TAU = prc.TAU

# every zkp_*_dev( of include/zkp_fk20.h has a row below or a written reason here
EXCLUDED = {}

VECTOR_KINDS = ("random", "holes", "identity", "constant", "spike")
POLY_KINDS = prc.POLY_KINDS + ("ends",)          # "ends": f_1 = .. = f_{N-2} = 0, the empty tail of c


class Lazy:
    """a sequence whose items are made on first use, and once: a replay takes all three sets of a build, a step of a call-order sequence
    one of them, and every point of a set costs an oracle multiplication"""

    def __init__(self, makers):
        self._makers, self._made = list(makers), {}

    def __len__(self):
        return len(self._makers)

    def __getitem__(self, i):
        i = operator.index(i)
        if i < 0:
            i += len(self._makers)
        if not 0 <= i < len(self._makers):
            raise IndexError(i)
        if i not in self._made:
            self._made[i] = self._makers[i]()
        return self._made[i]


def make_vector(kind, log2_n, flags, rng):
    """the exponents of one input vector.  holes: identity entries among random ones; constant: every butterfly of every stage meets
    A = T and A = -T, and the transform is the identity but for slot 0; spike: the transform is a single non-zero entry"""
    n = 1 << log2_n
    if kind == "identity":
        return [0] * n
    if kind == "constant":
        return [rng.randrange(1, R)] * n
    if kind == "spike":
        t = [0] * n
        t[rng.randrange(n)] = rng.randrange(1, R)
        return pm.ntt_flags(t, log2_n, flags ^ pm.INVERSE)
    v = [rng.randrange(1, R) for _ in range(n)]
    if kind == "holes":
        for i in range(0, n, 3):
            v[i] = 0
        v[n - 1] = 0
    return v


def ntt_io(vectors, log2_n, flags):
    """exponent vectors -> (points, inf) of the call and (out, out_inf) expected of it"""
    pts, inf = rc.expect_points(1, [e for v in vectors for e in v])
    out, out_inf = rc.expect_points(1, [e for v in vectors for e in pm.ntt_flags(v, log2_n, flags)])
    return pts, inf, out, out_inf


def make_poly(kind, n, rng):
    if kind == "ends":
        return [rng.randrange(1, R)] + [0] * (n - 2) + [rng.randrange(1, R)] if n > 1 else [rng.randrange(1, R)]
    return prc.make_poly(kind, n, rng)


def monomial_for(log2_n, tau=TAU):
    """([tau^k] g1 for k < N, by the oracle)"""
    return rc._cached(("fk20-monomial", log2_n, tau), lambda: rc.expect_points(1, [pow(tau, k, R) for k in range(1 << log2_n)])[0])


def fk20_setup_for(log2_n, tau=TAU):
    """(points, inf) expected of zkp_kzg_fk20_setup, by the oracle"""
    return rc._cached(("fk20-setup", log2_n, tau), lambda: rc.expect_points(1, fm.fk20_setup(tau, log2_n)))


def proofs_for(polys, log2_n, bitrev, tau=TAU):
    return rc.expect_points(1, [e for f in polys for e in fm.quotient_proofs(f, tau, log2_n, bitrev)])


def _ntt_sets(n_vec, log2_n, flags, seed):
    def build():
        rng = random.Random(seed * 419 + n_vec * 11 + log2_n * 5 + flags)
        # A: random holes identity; B: identity constant spike; C: spike random holes
        vecs = [[make_vector(VECTOR_KINDS[(2 * s + j) % 5], log2_n, flags, rng) for j in range(n_vec)] for s in range(3)]
        io = Lazy([(lambda v: lambda: ntt_io(v, log2_n, flags))(v) for v in vecs])
        return (Lazy([(lambda s: lambda: dict(points=io[s][0], inf=io[s][1]))(s) for s in range(3)]),
                Lazy([(lambda s: lambda: (io[s][2], io[s][3]))(s) for s in range(3)]))
    return rc._cached(("g1-ntt", n_vec, log2_n, flags, seed), build)


def _setup_sets(log2_n, seed):
    def build():
        rng = random.Random(seed * 53 + log2_n)
        taus = [TAU if s == 0 else rng.randrange(2, R) for s in range(3)]
        return (Lazy([(lambda t: lambda: dict(monomial=monomial_for(log2_n, t)))(t) for t in taus]),
                Lazy([(lambda t: lambda: fk20_setup_for(log2_n, t))(t) for t in taus]))
    return rc._cached(("fk20-setup-sets", log2_n, seed), build)


def _fk20_sets(n, log2_n, bitrev, seed):
    def build():
        rng = random.Random(seed * 211 + n * 13 + log2_n * 3 + bitrev)
        big_n = 1 << log2_n
        polys = [[make_poly(POLY_KINDS[(2 * s + j) % 5] if s else "random", big_n, rng) for j in range(n)] for s in range(3)]

        def inputs(f):
            setup, sinf = fk20_setup_for(log2_n)
            return dict(setup=setup, setup_inf=sinf, coeffs=fr_rows([v for p in f for v in p]))
        return (Lazy([(lambda f: lambda: inputs(f))(f) for f in polys]),
                Lazy([(lambda f: lambda: proofs_for(f, log2_n, bitrev))(f) for f in polys]))
    return rc._cached(("fk20-sets", n, log2_n, bitrev, seed), build)


CASES = [
    Case("g1_ntt-N64-x3-flags%d" % flags, ["zkp_g1_ntt_batch_dev"], "g1_ntt", lambda h, shape, seed: _ntt_sets(shape[0], shape[1], shape[2], seed),
         lambda e, t, sh: e.g1_ntt(t["points"], sh[1], inverse=bool(sh[2] & pm.INVERSE), bitrev=bool(sh[2] & pm.BITREV), inf=t["inf"]),
         (3, 6, flags), (1, 2, flags)) for flags in (pm.BITREV, pm.INVERSE)
] + [
    Case("kzg_fk20_setup-N64", ["zkp_kzg_fk20_setup_dev"], "kzg_fk20_setup", lambda h, shape, seed: _setup_sets(shape[0], seed),
         lambda e, t, sh: e.kzg_fk20_setup(t["monomial"], sh[0]), (6,), (2,)),
    Case("kzg_fk20-n3-N64-bitrev", ["zkp_kzg_fk20_batch_dev"], "kzg_fk20", lambda h, shape, seed: _fk20_sets(shape[0], shape[1], shape[2], seed),
         lambda e, t, sh: e.kzg_fk20(t["setup"], t["setup_inf"], t["coeffs"], sh[1], sh[2]), (3, 6, True), (1, 2, True)),
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
