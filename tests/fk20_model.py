"""The G1 NTT and the FK20 proofs on Python integers (exponents of the generator): the model the device calls of include/zkp_fk20.h are
compared with.  A G1 point [e] g1 is represented by e mod r, the identity by 0; the transforms are linear, so the G1 NTT of points is
poly_model.ntt of their exponents.  Nothing here imports the library under test."""
import poly_model as pm

R = pm.R
Z = 0xD201000000010000          # |z| of BLS12-381: r = z^4 - z^2 + 1
Z2 = Z * Z
assert R == Z2 * Z2 - Z2 + 1 and Z2 < 1 << 128


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def c_vector(f):
    """(f_{N-1}, 0 x (N + 1), f_1, .., f_{N-2}), of length 2N; N = 1: (f_0, 0)"""
    n = len(f)
    return [f[0], 0] if n == 1 else [f[n - 1]] + [0] * (n + 1) + list(f[1:n - 1])


def setup_vector(s):
    """(s_{N-2}, .., s_0, identity x (N + 1)), of length 2N, from the monomial setup s_k = tau^k"""
    n = len(s)
    return [s[n - 2 - e] for e in range(n - 1)] + [0] * (n + 1)


def fk20_setup(tau, log2_n):
    """the exponents of zkp_kzg_fk20_setup's 2N output points"""
    return pm.ntt(setup_vector([pow(tau, k, R) for k in range(1 << log2_n)]), log2_n + 1)


def h_vector(f, tau, log2_n):
    """the full inverse transform of size 2N of the slot-wise products (its first N entries are h)"""
    c_hat = pm.ntt(c_vector(f), log2_n + 1)
    return pm.ntt([a * b % R for a, b in zip(fk20_setup(tau, log2_n), c_hat)], log2_n + 1, inverse=True)


def fk20_proofs(f, tau, log2_n, bitrev=False):
    """the circulant pipeline of include/zkp_fk20.h: the exponents of the N proofs"""
    return pm.ntt(h_vector(f, tau, log2_n)[:1 << log2_n], log2_n, bitrev=bitrev)


def quotient_proofs(f, tau, log2_n, bitrev=False):
    """(f(tau) - f(w^m)) / (tau - w^m) for the domain point of every slot"""
    dom = pm.domain(log2_n)
    ft = horner(f, tau)
    out = []
    for m in range(1 << log2_n):
        x = dom[pm.bit_reverse(m, log2_n) if bitrev else m]
        out.append((ft - horner(f, x)) * pow(tau - x, -1, R) % R)
    return out


def lagrange_at(tau, log2_n):
    """l_i(tau) for the N-th roots of unity, from the definition"""
    n = 1 << log2_n
    dom = pm.domain(log2_n)
    scale = (pow(tau, n, R) - 1) * pow(n, -1, R) % R
    return [scale * d % R * pow(tau - d, -1, R) % R for d in dom]


def split(s):
    """s = a + b z^2 with a, b < z^2 < 2^128"""
    return s % Z2, s // Z2
