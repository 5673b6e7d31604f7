"""Python-integer model of the Groth16 producer side (include/zkp_prove.h; helper of test_prove_cpu.py, test_gpu_prove.py and
prove_replay_cases.py, not a test module): the sparse product, the evaluations of a witness, the quotient by the coset formula the
device uses, schoolbook division by X^N - 1 to check it against, and the exponents of a proof from the trapdoor.  `s` is the dict of
zkvm_pairings_amd.synthetic.groth16_circuit_secrets: rows as lists of (column, value), witnesses as lists of integers."""
import poly_model as pm

R = pm.R


def spmv(rows, x, n_cols=None):
    """out[k] = sum over row k of val x[col]; entries whose column is >= n_cols are dropped, as the device drops them"""
    return [sum(v * x[c] for c, v in row if n_cols is None or c < n_cols) % R for row in rows]


def evaluations(s, z):
    """a(w^k), b(w^k), c(w^k) for k < N: the three products, zero from n_rows on"""
    n = 1 << s["log2_n"]
    pad = [0] * (n - s["n_rows"])
    return tuple(spmv(s[name], z) + pad for name in ("rows_a", "rows_b", "rows_c"))


_quotients = {}


def quotient(s, z):
    """(h, sat): the N coefficients of the polynomial with h(7 w^i) = (a b - c)(7 w^i) / (7^N - 1), and whether a b == c on the domain
    (kept per circuit and witness: the tests ask again for every pair of blinding scalars)"""
    key = (id(s["rows_a"]), tuple(z))               # the rows are shared by the copies of a circuit that differ in their witnesses
    if key not in _quotients:
        _quotients[key] = (s["rows_a"], _quotient(s, z))      # held so that the id stays its own
    return _quotients[key][1]


def _quotient(s, z):
    k = s["log2_n"]
    n = 1 << k
    a, b, c = evaluations(s, z)
    sat = all(x * y % R == w for x, y, w in zip(a, b, c))
    ea, eb, ec = (pm.ntt(pm.ntt(v, k, inverse=True), k, coset=True) for v in (a, b, c))
    kinv = pow(pow(pm.GENERATOR, n, R) - 1, -1, R)
    h = pm.ntt([(x * y - w) * kinv % R for x, y, w in zip(ea, eb, ec)], k, inverse=True, coset=True)
    return h, sat


def poly_mul(p, q):
    out = [0] * (len(p) + len(q) - 1)
    for i, x in enumerate(p):
        if x:
            for j, y in enumerate(q):
                out[i + j] = (out[i + j] + x * y) % R
    return out


def divide_by_vanishing(p, n):
    """schoolbook division of the coefficient list p by X^n - 1 -> (quotient, remainder)"""
    rem = list(p)
    quo = [0] * max(0, len(p) - n)
    for i in range(len(p) - 1, n - 1, -1):
        lead = rem[i]
        quo[i - n] = lead
        rem[i] = 0
        rem[i - n] = (rem[i - n] + lead) % R
    return quo, rem[:n]


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def at_tau(s, z):
    """a(tau), b(tau), c(tau) of a witness from the QAP polynomials at tau"""
    return tuple(sum(zi * p for zi, p in zip(z, s[name])) % R for name in ("u_tau", "v_tau", "w_tau"))


def proof_exponents(s, z, r, t):
    """(e_A, e_B, e_C) of the proof of witness z with the blinding scalars r, t (the s of the issue), A = [e_A] g1 and so on.  The H sum uses
    the model's h coefficients below N - 1 (h_query has N - 1 entries), which for a satisfying witness is (a b - c)(tau) / t(tau)."""
    n, l = 1 << s["log2_n"], s["n_inputs"]
    alpha, beta, delta, tau = s["alpha"], s["beta"], s["delta"], s["tau"]
    dinv = pow(delta, -1, R)
    a_tau, b_tau, _ = at_tau(s, z)
    h, _ = quotient(s, z)
    h_tau = horner(h[:n - 1], tau)
    t_tau = (pow(tau, n, R) - 1) % R
    e_a = (alpha + a_tau + r * delta) % R
    e_b = (beta + b_tau + t * delta) % R
    priv = sum(z[i] * (beta * s["u_tau"][i] + alpha * s["v_tau"][i] + s["w_tau"][i]) for i in range(l + 1, s["m"])) % R
    e_c = (priv * dinv + h_tau * t_tau % R * dinv + t * e_a + r * e_b - r * t % R * delta) % R
    return e_a, e_b, e_c


def verifies(s, z, e_a, e_b, e_c):
    """the Groth16 verification equation in exponents: e_A e_B == alpha beta + vk_x gamma + e_C delta, vk_x from the public variables"""
    gamma, delta = s["gamma"], s["delta"]
    ginv = pow(gamma, -1, R)
    vkx = sum(z[i] * (s["beta"] * s["u_tau"][i] + s["alpha"] * s["v_tau"][i] + s["w_tau"][i]) for i in range(s["n_inputs"] + 1)) % R * ginv % R
    return e_a * e_b % R == (s["alpha"] * s["beta"] + vkx * gamma + e_c * delta) % R
