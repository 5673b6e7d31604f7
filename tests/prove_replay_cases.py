"""The capturable device-pointer entry points of include/zkp_prove.h (helper of test_gpu_prove_replay.py and test_prove_cpu.py; not a
test module): Case rows in the form of tests/replay_cases.py.  Expected values never come from the library under test: field values
are Python integers (tests/prove_model.py), and every point of a proof is [e] g for an exponent e computed from the circuit's
trapdoor (prove_model.proof_exponents), which is one oracle multiplication of the generator (replay_cases.expect_points).  The keys
themselves are inputs, made through a second engine that never captures.  The three sets of a case are three different circuits of one
shape (every row has two entries in A and in B), with their own keys, witnesses and blinding scalars."""
import random

import numpy as np

import prove_model as pmod
import replay_cases as rc
from replay_cases import Case, fr_rows

R = pmod.R

# every zkp_*_dev( of include/zkp_prove.h has a row below or a written reason here
EXCLUDED = {}

MATS = ("a", "b", "c")


def _mat_arrays(prefix, csr):
    row_ptr, col, val = csr
    return {prefix + "_row_ptr": row_ptr.view(np.int32), prefix + "_col": col.view(np.int32), prefix + "_val": val}


def _mat(t, prefix, n_rows, m):
    return (n_rows, m, t[prefix + "_row_ptr"], t[prefix + "_col"], t[prefix + "_val"])


def circuit_shape(log2_n):
    """(n_rows, m, n_inputs) of the replay circuits: one row short of the domain, m = N + 3"""
    n = 1 << log2_n
    return n - 1, n + 3, 1


def spmv_sets(n, log2_n, seed):
    def build():
        from zkvm_pairings_amd import synthetic
        n_rows, m, l = circuit_shape(log2_n)
        sets, exp = [], []
        for s in range(3):
            sec = synthetic.groth16_circuit_secrets(seed * 31 + s, log2_n, n_rows, m, l, n, row_lengths=[2] * n_rows)
            d = _mat_arrays("a", synthetic.csr_arrays(sec["rows_a"]))
            d["x"] = fr_rows([v for z in sec["z"] for v in z])
            sets.append(d)
            out = [v for z in sec["z"] for v in pmod.spmv(sec["rows_a"], z) + [0] * ((1 << log2_n) - n_rows)]
            exp.append((fr_rows(out),))
        return sets, exp
    return rc._cached(("spmv", n, log2_n, seed), build)


def _spmv_run(e, t, sh):
    n_rows, m, _ = circuit_shape(sh[1])
    return (e.fr_spmv(_mat(t, "a", n_rows, m), t["x"], out_stride=1 << sh[1]),)


def _circuit(h, n, log2_n, seed, s):
    from zkvm_pairings_amd import synthetic
    n_rows, m, l = circuit_shape(log2_n)
    bad = (n - 1,) if s == 1 else ()                    # set B: the last witness violates a constraint
    return synthetic.groth16_circuit_instance(seed * 37 + s, log2_n, n_rows, m, l, n, row_lengths=[2] * n_rows, bad=bad, engine=h)


def quotient_sets(h, n, log2_n, seed):
    def build():
        sets, exp = [], []
        for s in range(3):
            r1cs, _, _, wit, sec = _circuit(h, n, log2_n, seed, s)
            d = {}
            for name, csr in zip(MATS, (r1cs.a, r1cs.b, r1cs.c)):
                d.update(_mat_arrays(name, csr))
            d["witness"] = wit.reshape(-1, 4)
            sets.append(d)
            hs, sat = zip(*(pmod.quotient(sec, z) for z in sec["z"]))
            exp.append((fr_rows([v for x in hs for v in x]), np.array(sat, dtype=np.uint8)))
        return sets, exp
    return rc._cached(("quotient", n, log2_n, seed), build)


def _quotient_run(e, t, sh):
    n_rows, m, l = circuit_shape(sh[1])
    return e.groth16_quotient(sh[1], l, *(_mat(t, x, n_rows, m) for x in MATS), t["witness"])


PK_ARRAYS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "a_query", "a_inf", "b_g1_query", "b_g1_inf", "b_g2_query", "b_g2_inf", "l_query", "l_inf",
             "h_query")


def expected_proofs(sec, rs):
    """((A, inf_a, B, inf_b, C, inf_c), sat) of every witness of `sec` under the blinding pairs rs, from the trapdoor and the oracle"""
    ea, eb, ec, sat = [], [], [], []
    for z, (r, t) in zip(sec["z"], rs):
        x, y, w = pmod.proof_exponents(sec, z, r, t)
        ea.append(x)
        eb.append(y)
        ec.append(w)
        sat.append(1 if pmod.quotient(sec, z)[1] else 0)
    (a, ia), (b, ib), (c, ic) = rc.expect_points(1, ea), rc.expect_points(2, eb), rc.expect_points(1, ec)
    return (a, ia, b, ib, c, ic), np.array(sat, dtype=np.uint8)


def prove_sets(h, n, log2_n, seed):
    def build():
        sets, exp = [], []
        for s in range(3):
            rng = random.Random(seed * 41 + s)
            r1cs, pk, _, wit, sec = _circuit(h, n, log2_n, seed, s)
            d = {}
            for name, csr in zip(MATS, (r1cs.a, r1cs.b, r1cs.c)):
                d.update(_mat_arrays(name, csr))
            d.update({"pk_" + name: x for name, x in pk.arrays().items()})
            d["witness"] = wit.reshape(-1, 4)
            rs = [(0, 0) if s == 2 and j == 0 else (rng.randrange(R), rng.randrange(R)) for j in range(n)]
            d["rs"] = fr_rows([v for p in rs for v in p])
            sets.append(d)
            pts, sat = expected_proofs(sec, rs)
            exp.append(pts + (sat,))
        return sets, exp
    return rc._cached(("prove", n, log2_n, seed), build)


def _prove_run(e, t, sh):
    n_rows, m, l = circuit_shape(sh[1])
    return e.groth16_prove(sh[1], l, *(_mat(t, x, n_rows, m) for x in MATS), {name: t["pk_" + name] for name in PK_ARRAYS}, t["witness"], t["rs"])


# N = 64 and N = 4 as log2
CASES = [
    Case("fr_spmv-n3-N64", ["zkp_fr_spmv_batch_dev"], "fr_spmv", lambda h, shape, seed: spmv_sets(shape[0], shape[1], seed), _spmv_run, (3, 6), (1, 2)),
    Case("groth16_quotient-n3-N64", ["zkp_groth16_quotient_batch_dev"], "groth16_quotient", lambda h, shape, seed: quotient_sets(h, shape[0], shape[1], seed),
         _quotient_run, (3, 6), (1, 2)),
    Case("groth16_prove-n3-N64", ["zkp_groth16_prove_batch_dev"], "groth16_prove", lambda h, shape, seed: prove_sets(h, shape[0], shape[1], seed), _prove_run,
         (3, 6), (1, 2)),
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
