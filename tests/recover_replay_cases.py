"""The device-pointer entry point of include/zkp_recover.h (helper of test_gpu_recover_replay.py, test_gpu_recover.py,
test_gpu_call_order_recover.py and test_recover_cpu.py; not a test module): the Case row in the form of tests/replay_cases.py, and the
instances the recovery tests share.  Expected values never come from the library under test: a consistent blob must come back as the
polynomial its cells were made from (poly_model's transform of the coefficients), a blob with too few cells as zeros, and a corrupted
blob with exactly M / 2 cells as what tests/recover_model.py computes on Python integers - test_recover_cpu.py holds that model to
Lagrange's formula."""
import random

import numpy as np

import poly_model as pm
import recover_model as rm
import recover_shapes as rs
import replay_cases as rc
from replay_cases import Case, fr_rows

R = pm.R

# every zkp_*_dev( of include/zkp_recover.h has a row below or a written reason here
EXCLUDED = {}

# what a blob of an instance is: an erasure pattern of recover_model.PATTERNS, or
#   few        M / 2 - 1 cells present: a zero row, ok = 0
#   half-bad   exactly M / 2 cells, one value corrupted: ok = 1 and the other interpolant
#   more-bad   M / 2 + 1 cells, one value corrupted: ok = 0, the row unspecified but canonical (expected row: None)
KINDS = rm.PATTERNS + ("few", "half-bad", "more-bad")


def garbage(rng, l):
    """the row of a missing cell: bytes nobody may interpret, every word above r's top word"""
    return [(1 << 256) - 1 - rng.randrange(1 << 64) for _ in range(l)]


def blob(kind, log2_n, log2_l, bitrev, rng):
    """(rows: M lists of l integers, present: M flags, expected coefficients or None, expected ok)"""
    n, l, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
    f = [rng.randrange(R) for _ in range(n)]
    cells = rm.cells_of(f, log2_n, log2_l, bitrev)
    want, ok = f, 1
    if kind in rm.PATTERNS:
        present = rm.pattern(kind, big_m, rng)
    else:
        keep = {"few": k - 1, "half-bad": k, "more-bad": k + 1}[kind]
        order = list(range(big_m))
        rng.shuffle(order)
        present = [1 if m in set(order[:keep]) else 0 for m in range(big_m)]
        if kind == "few":
            want, ok = [0] * n, 0
        else:
            m, u = order[0], rng.randrange(l)
            cells[m][u] = (cells[m][u] + 1 + rng.randrange(R - 1)) % R
            if kind == "half-bad":
                want, ok = rm.recover(cells, present, log2_n, log2_l, bitrev)
                assert ok == 1 and want != f
            else:
                want, ok = None, 0
    rows = [cells[m] if present[m] else garbage(rng, l) for m in range(big_m)]
    return rows, present, want, ok


def instance(kinds, log2_n, log2_l, bitrev, seed):
    """one blob per entry of kinds -> dict(values (n M l, 4), present (n M,), coeffs (n N, 4), ok (n,) int32, free: the blobs whose row is
    unspecified)"""
    def build():
        rng = random.Random(seed * 131 + log2_n * 17 + log2_l * 5 + bitrev)
        n_co = 1 << log2_n
        vals, pres, co, oks, free = [], [], [], [], []
        for j, kind in enumerate(kinds):
            rows, present, want, ok = blob(kind, log2_n, log2_l, bitrev, rng)
            vals += [v for row in rows for v in row]
            pres += present
            if want is None:
                free.append(j)
                want = [0] * n_co
            co += want
            oks.append(ok)
        return dict(values=fr_rows(vals), present=np.array(pres, dtype=np.uint8), coeffs=fr_rows(co), ok=np.array(oks, dtype=np.int32), free=free)
    return rc._cached(("recover-instance", tuple(kinds), log2_n, log2_l, bitrev, seed), build)


def below_r(rows):
    """every (.., 4) uint64 row is a canonical element"""
    return all(int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 < R for a, b, c, d in np.asarray(rows).reshape(-1, 4))


def check(got_coeffs, got_ok, inst, what=""):
    """the outputs of a call against an instance: flags all, rows byte for byte but for the unspecified ones, which must be canonical"""
    co, ok = np.asarray(got_coeffs), np.asarray(got_ok)
    n = inst["ok"].size
    assert ok.dtype == np.int32 and ok.tobytes() == inst["ok"].tobytes(), (what, ok.tolist(), inst["ok"].tolist())
    co, want = co.reshape(n, -1), inst["coeffs"].reshape(n, -1)
    assert co.shape == want.shape and co.dtype == want.dtype, (what, co.shape, want.shape)
    for j in range(n):
        if j in inst["free"]:
            assert below_r(co[j]), (what, j)
        else:
            assert co[j].tobytes() == want[j].tobytes(), "%s: blob %d of %d differs" % (what, j, n)


# ---- one call across a slice boundary, assembled as slice_pools' calls are: a pool of 11 blobs, a seeded index sequence over it, the short
# last slice made of pool items used nowhere else in the call
SLICE_B, SLICE_TAIL = 11, (7, 9, 10)
SLICE_KINDS = ("random-half", "none", "few", "even", "half-bad", "one", "odd", "first-half", "random-half", "few", "second-half")


def slice_call(bitrev):
    import slice_pools as sp
    p = instance(SLICE_KINDS, rs.SLICE_LOG2_N, rs.SLICE_LOG2_L, bitrev, sp.SEED)
    idx = sp.draw(sp.SEED + 501 + bitrev, rs.SLICE_N, SLICE_TAIL, SLICE_B)
    n_co, big_m = 1 << rs.SLICE_LOG2_N, 2 << (rs.SLICE_LOG2_N - rs.SLICE_LOG2_L)
    per_v = big_m << rs.SLICE_LOG2_L
    return sp.Call(rs.SLICE_N, rs.SLICE_LEN, idx,
                   dict(values=(sp.take(p["values"], SLICE_B, idx), per_v), present=(sp.take(p["present"], SLICE_B, idx), big_m)),
                   dict(coeffs=(sp.take(p["coeffs"], SLICE_B, idx), n_co), ok=(sp.take(p["ok"], SLICE_B, idx), 1)), p)


# ---- the replay case: three sets of the same shape whose polynomials AND erasure patterns differ; B holds a blob with too few cells,
# C one with exactly M / 2 cells and a corrupted value
SET_KINDS = (("random-half", "even", "one"), ("first-half", "few", "random-half"), ("half-bad", "odd", "second-half"))


def _recover_sets(n, log2_n, log2_l, bitrev, seed):
    insts = [instance(tuple(SET_KINDS[s][j % 3] for j in range(n)), log2_n, log2_l, bitrev, seed + 7 * s) for s in range(3)]
    return [dict(values=i["values"], present=i["present"]) for i in insts], [(i["coeffs"], i["ok"]) for i in insts]


# shape: (n, log2_n, log2_l, bitrev)
CASES = [
    Case("das_recover-n3-N16-l4-bitrev", ["zkp_das_recover_batch_dev"], "das_recover", lambda h, shape, seed: _recover_sets(*shape, seed),
         lambda e, t, sh: e.das_recover(t["values"], t["present"], sh[1], sh[2], sh[3]), (3, 4, 2, True), (1, 2, 1, True)),
    Case("das_recover-n2-N64-l1", ["zkp_das_recover_batch_dev"], "das_recover", lambda h, shape, seed: _recover_sets(*shape, seed),
         lambda e, t, sh: e.das_recover(t["values"], t["present"], sh[1], sh[2], sh[3]), (2, 6, 0, False), (1, 1, 0, False)),
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
