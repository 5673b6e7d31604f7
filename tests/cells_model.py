"""The KZG cell proofs on Python integers (exponents of the generator): the model the device calls of include/zkp_cells.h are compared
with.  A G1 point [e] g1 is represented by e mod r, the identity by 0, as in fk20_model.py.  Two routes to every figure: the DEFINITION
(cells as evaluations on cosets, proofs as quotients by X^l - c^l, the interpolant by Lagrange's formula) and the PIPELINE of the header
(stride vectors, transforms of size 2 k, slot-wise multiply-accumulate, transforms of size 2 k and M).  Nothing here imports the library
under test."""
import fk20_model as fm
import poly_model as pm

R = pm.R
horner = fm.horner


def sizes(log2_n, log2_l, log2_ext):
    """(N, l, k, D, M)"""
    n, l = 1 << log2_n, 1 << log2_l
    return n, l, n // l, n << log2_ext, (n << log2_ext) // l


def coset_shift(m, log2_n, log2_l, log2_ext, bitrev):
    """c_m = w_D^m', m' = bitrev_M(m) under bitrev"""
    log2_d = log2_n + log2_ext
    mp = pm.bit_reverse(m, log2_d - log2_l) if bitrev else m
    return pm.domain(log2_d)[mp]


def cell_points(m, log2_n, log2_l, log2_ext, bitrev):
    """the l points of cell m in the order of its values: c_m w_l^u', u' = bitrev_l(u) under bitrev"""
    c, dom_l = coset_shift(m, log2_n, log2_l, log2_ext, bitrev), pm.domain(log2_l)
    return [c * dom_l[pm.bit_reverse(u, log2_l) if bitrev else u] % R for u in range(1 << log2_l)]


# ------------------------------------------------------------------------------------------------------------------- the definition
def cell_values(f, log2_n, log2_l, log2_ext, bitrev):
    """M rows of l values, from the definition"""
    _, _, _, _, big_m = sizes(log2_n, log2_l, log2_ext)
    return [[horner(f, x) for x in cell_points(m, log2_n, log2_l, log2_ext, bitrev)] for m in range(big_m)]


def quotient_by_power(f, l, a):
    """(q, rem) with f = q (X^l - a) + rem, deg rem < l"""
    rem = list(f)
    q = [0] * max(len(f) - l, 0)
    for d in range(len(f) - 1, l - 1, -1):
        q[d - l] = rem[d]
        rem[d - l] = (rem[d - l] + rem[d] * a) % R
        rem[d] = 0
    return q, rem[:l]


def quotient_proofs(f, tau, log2_n, log2_l, log2_ext, bitrev=False):
    """q_m(tau) for q_m = (f - I_m) / (X^l - c_m^l), I_m = f mod (X^l - c_m^l), for every cell m"""
    _, l, _, _, big_m = sizes(log2_n, log2_l, log2_ext)
    out = []
    for m in range(big_m):
        a = pow(coset_shift(m, log2_n, log2_l, log2_ext, bitrev), l, R)
        out.append(horner(quotient_by_power(f, l, a)[0], tau))
    return out


def lagrange_at(points, values, x):
    """the interpolant of (points, values) at x, by Lagrange's formula"""
    acc = 0
    for i, (p, v) in enumerate(zip(points, values)):
        num = den = 1
        for j, q in enumerate(points):
            if j != i:
                num, den = num * (x - q) % R, den * (p - q) % R
        acc = (acc + v * num % R * pow(den, -1, R)) % R
    return acc


def cell_holds(commitment, m, values, proof, tau, log2_n, log2_l, log2_ext, bitrev):
    """e(C - [I(tau)] g1 + [c^l] pi, g2) == e(pi, [tau^l] g2), on exponents"""
    l = 1 << log2_l
    pts = cell_points(m, log2_n, log2_l, log2_ext, bitrev)
    c_l = pow(coset_shift(m, log2_n, log2_l, log2_ext, bitrev), l, R)
    return (commitment - lagrange_at(pts, values, tau) + c_l * proof) % R == proof * pow(tau, l, R) % R


# ------------------------------------------------------------------------------------------------------------------- the pipeline
def stride_poly(f, i, log2_l):
    """g_d = f_{(d + 1) l - 1 - i}, d < k: the coefficients stride i sees"""
    l = 1 << log2_l
    return [f[(d + 1) * l - 1 - i] for d in range(len(f) // l)]


def c_vectors(f, log2_l):
    """c_i = (f_{N-1-i}, 0 x (k + 1), f_{2l-1-i}, .., f_{N-l-1-i}) for every stride i < l; k = 1: (f_{N-1-i}, 0)"""
    return [fm.c_vector(stride_poly(f, i, log2_l)) for i in range(1 << log2_l)]


def setup_vectors(s, log2_l):
    """(s_{N-l-1-i}, s_{N-2l-1-i}, .., k - 1 entries, then k + 1 identities) for every stride i < l"""
    l = 1 << log2_l
    k = len(s) // l
    return [[s[(k - 1 - e) * l - 1 - i] for e in range(k - 1)] + [0] * (k + 1) for i in range(l)]


def cells_setup(tau, log2_n, log2_l):
    """the exponents of zkp_kzg_cells_setup's output: l vectors of 2 k"""
    s = [pow(tau, j, R) for j in range(1 << log2_n)]
    return [pm.ntt(v, log2_n - log2_l + 1) for v in setup_vectors(s, log2_l)]


def h_vector(f, tau, log2_n, log2_l):
    """the full inverse transform of size 2 k of the slot-wise sums (its first k entries are h)"""
    k1 = log2_n - log2_l + 1
    x = cells_setup(tau, log2_n, log2_l)
    c_hat = [pm.ntt(c, k1) for c in c_vectors(f, log2_l)]
    acc = [sum(xi[t] * ci[t] for xi, ci in zip(x, c_hat)) % R for t in range(1 << k1)]
    return pm.ntt(acc, k1, inverse=True)


def cell_proofs(f, tau, log2_n, log2_l, log2_ext, bitrev=False):
    """the pipeline of include/zkp_cells.h: the exponents of the M proofs"""
    _, _, k, _, big_m = sizes(log2_n, log2_l, log2_ext)
    h = h_vector(f, tau, log2_n, log2_l)[:k]
    return pm.ntt(h + [0] * (big_m - k), log2_n - log2_l + log2_ext, bitrev=bitrev)


def extended_values(f, log2_n, log2_l, log2_ext, bitrev):
    """the cells through the Fr transform of the zero-padded coefficients, cut into rows of l (the bit-reversed layout only)"""
    n, l, _, d, big_m = sizes(log2_n, log2_l, log2_ext)
    ev = pm.ntt(list(f) + [0] * (d - n), log2_n + log2_ext, bitrev=bitrev)
    return [ev[l * m:l * m + l] for m in range(big_m)]


def interpolant_coefficients(values, m, log2_n, log2_l, log2_ext, bitrev):
    """the verifier's route: the inverse transform of size l, then coefficient i times c_m^-i"""
    ci = pow(coset_shift(m, log2_n, log2_l, log2_ext, bitrev), -1, R)
    return [v * pow(ci, i, R) % R for i, v in enumerate(pm.ntt(values, log2_l, inverse=True, bitrev=bitrev))]


def batch_holds(cells, rs, tau, log2_n, log2_l, log2_ext, bitrev):
    """the combined equation of zkp_kzg_cell_verify_batch on exponents; cells: (commitment, m, values, proof) each, rs: the r_j"""
    l = 1 << log2_l
    a = [0] * l
    lhs = rhs = 0
    for (cm, m, values, proof), r in zip(cells, rs):
        for i, v in enumerate(interpolant_coefficients(values, m, log2_n, log2_l, log2_ext, bitrev)):
            a[i] = (a[i] + r * v) % R
        c_l = pow(coset_shift(m, log2_n, log2_l, log2_ext, bitrev), l, R)
        lhs = (lhs + r * proof) % R
        rhs = (rhs + r * cm + r * c_l % R * proof) % R
    rhs = (rhs - sum(ai * pow(tau, i, R) for i, ai in enumerate(a))) % R
    return lhs * pow(tau, l, R) % R == rhs


# ------------------------------------------------------------------------------------------------------------------- the additions' cases
def addition_cases(f, tau, log2_n, log2_l, s):
    """k_cell_mac and k_cell_sum replayed on exponents for one polynomial with groups of g = 2^s strides: which exceptional cases of the
    group law their additions meet.  The scalars are the device's (the transform of c_i / (2 k)), the chain is the kernel's: bits 255 .. 0,
    a doubling per bit, then base q = 0 .. g - 1 added where scalar q has the bit.  -> counts of: mac_double (accumulator == +X, finite),
    mac_opposite (== -X), mac_into_infinity (accumulator infinite), sum_double, sum_opposite, sum_infinite (either operand)"""
    k1, l, g = log2_n - log2_l + 1, 1 << log2_l, 1 << s
    ninv = pow(1 << k1, -1, R)
    x = cells_setup(tau, log2_n, log2_l)
    c_hat = [pm.ntt([v * ninv % R for v in c], k1) for c in c_vectors(f, log2_l)]
    out = dict(mac_double=0, mac_opposite=0, mac_into_infinity=0, sum_double=0, sum_opposite=0, sum_infinite=0)
    for t in range(1 << k1):
        partials = []
        for i0 in range(0, l, g):
            live = [q for q in range(g) if x[i0 + q][t]]                  # a base flagged infinite has its bits masked away
            acc = 0
            for bit in range(255, -1, -1):
                acc = 2 * acc % R
                for q in live:
                    if (c_hat[i0 + q][t] >> bit) & 1:
                        base = x[i0 + q][t]
                        key = "mac_into_infinity" if acc == 0 else "mac_double" if acc == base else "mac_opposite" if (acc + base) % R == 0 else None
                        if key:
                            out[key] += 1
                        acc = (acc + base) % R
            assert acc == sum(c_hat[i0 + q][t] * x[i0 + q][t] for q in range(g)) % R
            partials.append(acc)
        acc = partials[0]
        for p in partials[1:]:
            key = "sum_infinite" if acc == 0 or p == 0 else "sum_double" if acc == p else "sum_opposite" if (acc + p) % R == 0 else None
            if key:
                out[key] += 1
            acc = (acc + p) % R
    return out
