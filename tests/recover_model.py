"""The cell recovery of include/zkp_recover.h on Python integers (helper of test_recover_cpu.py and of the GPU tests; not a test module):
the pipeline of the header - the interpolants' coefficients column by column, one vanishing polynomial per blob, three transforms of size
M per column - and the erasure patterns the tests share.  The extension is 2 throughout: D = 2 N, M = D / l."""
import random

import cells_model as cm
import poly_model as pm

R = pm.R
PATTERNS = ("none", "one", "first-half", "second-half", "even", "odd", "random-half")


def sizes(log2_n, log2_l):
    """(N, l, k, D, M, mu)"""
    n, l, k, d, big_m = cm.sizes(log2_n, log2_l, 1)
    return n, l, k, d, big_m, log2_n + 1 - log2_l


def cells_of(f, log2_n, log2_l, bitrev):
    """the M x l values of f in cell order, through ONE transform of size D: under bitrev the rows of the bit-reversed extended blob,
    otherwise value u of cell m is entry m + M u of the natural-order one"""
    n, l, _, d, big_m, _ = sizes(log2_n, log2_l)
    ev = pm.ntt(list(f) + [0] * (d - n), log2_n + 1, bitrev=bitrev)
    if bitrev:
        return [ev[l * m:l * m + l] for m in range(big_m)]
    return [[ev[m + big_m * u] for u in range(l)] for m in range(big_m)]


def pattern(kind, big_m, rng=None):
    """the present mask of a named erasure pattern over M cells (1: received)"""
    half = big_m // 2
    if kind == "none":
        return [1] * big_m
    if kind == "one":
        return [0 if m == big_m - 1 else 1 for m in range(big_m)]
    if kind == "first-half":
        return [0] * half + [1] * half
    if kind == "second-half":
        return [1] * half + [0] * half
    if kind == "even":
        return [m & 1 for m in range(big_m)]
    if kind == "odd":
        return [1 - (m & 1) for m in range(big_m)]
    assert kind == "random-half", kind
    gone = set((rng or random.Random(big_m)).sample(range(big_m), half))
    return [0 if m in gone else 1 for m in range(big_m)]


def vanishing(missing, mu):
    """the coefficients of prod (Y - w_M^m') over the exponents in `missing`, zero-padded to M, one linear factor at a time"""
    dom = pm.domain(mu)
    z = [1] + [0] * ((1 << mu) - 1)
    for deg, mp in enumerate(missing):
        w = dom[mp]
        z = [((z[d - 1] if d else 0) - w * z[d]) % R if d <= deg + 1 else 0 for d in range(1 << mu)]
    return z


def recover(values, present, log2_n, log2_l, bitrev):
    """values: M rows of l integers (the row of a missing cell is never looked at: it may be None), present: M flags.
    -> (the N coefficients, ok) exactly as zkp_das_recover_batch leaves them for a consistent or an underdetermined blob"""
    n, l, k, _, _, _ = sizes(log2_n, log2_l)
    cols = decode(values, present, log2_n, log2_l, bitrev)
    if cols is None:
        return [0] * n, 0
    f = [0] * n
    for i, p in enumerate(cols):
        for t in range(k):
            f[i + l * t] = p[t]
    return f, 0 if any(any(p[k:]) for p in cols) else 1


def decode(values, present, log2_n, log2_l, bitrev):
    """the l decoded columns p (M entries each: p_t is f_{i + l t} for t < M / 2, the tail behind it is zero iff the cells are consistent),
    or None when fewer than M / 2 cells are present"""
    n, l, k, _, big_m, mu = sizes(log2_n, log2_l)
    assert len(values) == len(present) == big_m
    if sum(1 for p in present if p) < k:
        return None
    mp = [pm.bit_reverse(m, mu) if bitrev else m for m in range(big_m)]
    z = vanishing([mp[m] for m in range(big_m) if not present[m]], mu)
    zr, zs = pm.ntt(z, mu), pm.ntt(z, mu, coset=True)
    zs_inv = [pow(v, -1, R) for v in zs]
    cols = [[0] * big_m for _ in range(l)]
    for m in range(big_m):
        if present[m]:
            for i, v in enumerate(cm.interpolant_coefficients(values[m], m, log2_n, log2_l, 1, bitrev)):
                cols[i][mp[m]] = v * zr[mp[m]] % R
    out = []
    for col in cols:
        q = pm.ntt(col, mu, inverse=True)
        out.append(pm.ntt([a * b % R for a, b in zip(pm.ntt(q, mu, coset=True), zs_inv)], mu, inverse=True, coset=True))
    return out


def interpolant_of_half(values, present, log2_n, log2_l, bitrev):
    """for exactly M / 2 present cells: the unique polynomial of degree below N through them, by Lagrange's formula (the definition)"""
    n, l, k, _, big_m, _ = sizes(log2_n, log2_l)
    pts, vals = [], []
    for m in range(big_m):
        if present[m]:
            pts += cm.cell_points(m, log2_n, log2_l, 1, bitrev)
            vals += list(values[m])
    assert len(pts) == n
    coeffs = [0] * n
    for j, (xj, yj) in enumerate(zip(pts, vals)):
        num, den = [1], 1                       # prod_{i != j} (X - x_i), coefficient list, low first
        for i, xi in enumerate(pts):
            if i != j:
                num = [((num[d - 1] if d else 0) - xi * (num[d] if d < len(num) else 0)) % R for d in range(len(num) + 1)]
                den = den * (xj - xi) % R
        s = yj * pow(den, -1, R) % R
        for d in range(n):
            coeffs[d] = (coeffs[d] + s * num[d]) % R
    return coeffs
