"""The shapes the sparse product, the quotient and the prover are tested on (helper of test_prove_cpu.py and test_gpu_prove.py, not a
test module).  The product's matrices are chosen so that EVERY lane count 2^t the planner (csrc/zkp_prove_plan.hpp: spmv_t) can pick
is hit: t is the smallest with 2^t >= ceil(nnz / n_rows), at most 6.  test_prove_cpu.py asserts the coverage from the plan program's
output for this table; nothing here needs a GPU."""
import random

import numpy as np

import prove_model as pmod
from replay_cases import fr_rows

R = pmod.R

# name -> (row lengths, n_cols): "mixed" holds rows of 0, 1, 2, 63, 64, 65, 300 and 1025 entries (mean 190: t = 6); the uniform ones
# have 65 rows (more than one lane group per workgroup at every t, an odd count) of 1, 2, 3, 7, 16, 32 entries: t = 0 .. 5
SPMV = {
    "mixed": ([0, 1, 2, 63, 64, 65, 300, 1025], 97),
    "len1": ([1] * 65, 33),
    "len2": ([2] * 65, 33),
    "len3": ([3] * 65, 33),
    "len7": ([7] * 65, 33),
    "len16": ([16] * 65, 33),
    "len32": ([32] * 65, 70),
    "one_row": ([5], 9),
    "no_rows": ([], 9),
}
SPMV_N = (1, 3)


def expected_t(lengths):
    mean = -(-sum(lengths) // len(lengths)) if lengths else 0
    t = 0
    while t < 6 and (1 << t) < mean:
        t += 1
    return t


def spmv_matrix(name):
    """rows as lists of (column, value): values from {0, 1, r - 1, random}, and a repeated column inside every row of two or more"""
    lengths, n_cols = SPMV[name]
    rng = random.Random("spmv-" + name)
    rows = []
    for ln in lengths:
        row = [(rng.randrange(n_cols), (0, 1, R - 1, rng.randrange(R))[rng.randrange(4)]) for _ in range(ln)]
        if ln >= 2:
            row[-1] = (row[0][0], rng.randrange(1, R))
        rows.append(row)
    return rows, n_cols


def spmv_vectors(name, n):
    _, n_cols = SPMV[name]
    rng = random.Random("spmv-x-%s-%d" % (name, n))
    xs = [[(0, 1, R - 1, rng.randrange(R), rng.randrange(R))[rng.randrange(5)] for _ in range(n_cols)] for _ in range(n)]
    return xs


def csr(rows):
    from zkvm_pairings_amd import synthetic
    return synthetic.csr_arrays(rows)


def spmv_expected(rows, xs, out_stride):
    """(n, out_stride, 4) uint64 from Python integers: the product and the zero padding"""
    out = []
    for x in xs:
        out += pmod.spmv(rows, x) + [0] * (out_stride - len(rows))
    return fr_rows(out).reshape(len(xs), out_stride, 4) if out else np.zeros((len(xs), out_stride, 4), dtype=np.uint64)


# the quotient: one pass (N <= 2^10), the tile boundary, two passes; full, one short and a single row
QUOTIENT_LOG2 = (1, 2, 5, 10, 11)


def quotient_rows(log2_n):
    n = 1 << log2_n
    return sorted(set((n, n - 1, 1)))


# the prover: (log2_n, n_inputs, n); m = N + 3
PROVER = [(k, l, n) for k in (2, 6, 11) for l in (0, 1, 5) for n in (1, 5)]
SLICES = dict(log2_n=10, m=1027, n=4100)
