#!/usr/bin/env python3
"""Derive every curve/tower constant from first principles (Python big ints) and emit
  oracle/orc_constants.h                     64-bit Montgomery limbs (R = 2^384) for the C oracle
  zkvm_pairings_amd/csrc/zkp_constants.h    32-bit Montgomery limbs (R = 2^384) for the HIP kernels
Both files are committed; re-run this script only to regenerate them.  The numbers are mathematical
facts (p, r, x, generators, xi^((p-1)k/6), psi coefficients) - nothing is read from the reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import bls12_381_model as m  # noqa: E402

P = m.P
R384 = (1 << 384) % P


def mont(v):
    return v * R384 % P


def limbs(v, bits, n):
    return [(v >> (bits * i)) & ((1 << bits) - 1) for i in range(n)]


def c_arr64(v):
    return "{" + ", ".join("0x%016xULL" % x for x in limbs(v, 64, 6)) + "}"


def c_arr32(v):
    return "{" + ", ".join("0x%08xu" % x for x in limbs(v, 32, 12)) + "}"


def consts():
    xi = m.XI
    g = [m.f2_pow(xi, i * (P - 1) // 6) for i in range(6)]
    out = {}
    out["P"] = P
    out["R"] = R384                     # Montgomery one
    out["R2"] = R384 * R384 % P
    out["B"] = 4
    out["G1_X"], out["G1_Y"] = m.G1_GEN
    out["G2_X0"], out["G2_X1"] = m.G2_GEN[0]
    out["G2_Y0"], out["G2_Y1"] = m.G2_GEN[1]
    out["BETA"] = m.BETA
    # true Frobenius: Fp6 c1 *= xi^((p-1)/3), c2 *= xi^(2(p-1)/3); Fp12 c1 *= xi^((p-1)/6)
    out["FROB6_C1_0"], out["FROB6_C1_1"] = g[2]
    out["FROB6_C2_0"], out["FROB6_C2_1"] = g[4]
    out["FROB12_C1_0"], out["FROB12_C1_1"] = g[1]
    # per-w-power coefficients gamma_i = xi^(i(p-1)/6) for i = 1..5 (flat Frobenius)
    for i in range(1, 6):
        out["GAMMA%d_0" % i], out["GAMMA%d_1" % i] = g[i]
    # what the reference multiplies by in Fp6::frobenius_map (src/fp6.rs:150-171) - refcompat only
    out["REF_FROB6_C1"] = m.REF_FROB6_C1
    out["REF_FROB6_C2"] = m.REF_FROB6_C2
    out["PSI_X_0"], out["PSI_X_1"] = m.PSI_X
    out["PSI_Y_0"], out["PSI_Y_1"] = m.PSI_Y
    return out


# ---------------------------------------------------------------------------------------------------- hash-to-G2 (RFC 9380, zkp_bls.hip)
H2C_A = (0, 240)                  # E': y^2 = x^3 + 240 i x + 1012 (1 + i)
H2C_B = (1012, 1012)
H2C_Z = (P - 2, P - 1)            # -(2 + i)
H2C_KERNEL_X = (P - 6, 6)         # -6 + 6 i: the abscissa of the 3-isogeny's kernel


def f2_sqrt(a):
    """a square root in Fp2 (p = 3 mod 4), or None"""
    if a == (0, 0):
        return a
    a0, a1 = a
    if a1 == 0:
        s = m.fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = m.fp_sqrt(-a0 % P)
        return None if s is None else (0, s)
    n = m.fp_sqrt((a0 * a0 + a1 * a1) % P)
    if n is None:
        return None
    for t in ((a0 + n) * (P + 1) // 2 % P, (a0 - n) * (P + 1) // 2 % P):
        c = m.fp_sqrt(t)
        if c is not None:
            r = (c, a1 * m.fp_inv(2 * c % P) % P)
            return r if m.f2_sqr(r) == a else None
    return None


def f2_cbrt(t):
    """a cube root in Fp2, or None: t^alpha with 3 alpha = 1 mod the 3-free part of p^2 - 1, corrected inside the 3-Sylow subgroup"""
    q1, k = P * P - 1, 0
    while q1 % 3 == 0:
        q1, k = q1 // 3, k + 1
    assert k <= 6
    g, nr = (1, 0), (1, 1)
    while m.f2_pow(g, 3 ** (k - 1)) == (1, 0):          # a generator of the 3-Sylow subgroup
        nr = m.f2_add(nr, (1, 0))
        g = m.f2_pow(nr, q1)
    c = m.f2_pow(t, pow(3, -1, q1))
    h = (1, 0)
    for _ in range(3 ** k):
        r = m.f2_mul(c, h)
        if m.f2_mul(m.f2_sqr(r), r) == t:
            return r
        h = m.f2_mul(h, g)
    return None


def _pmul(a, b):
    out = [(0, 0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = m.f2_add(out[i + j], m.f2_mul(x, y))
    return out


def _padd(a, b):
    n = max(len(a), len(b))
    a, b = a + [(0, 0)] * (n - len(a)), b + [(0, 0)] * (n - len(b))
    return [m.f2_add(x, y) for x, y in zip(a, b)]


def h2c_isogeny_candidates():
    """Velu's formulas for the kernel {O, (x0, +-y0)} of E', then the six scalings (x, y) -> (x / s^2, y / s^3) that land on
    y^2 = x^3 + 4 (1 + i).  Each candidate is (x_num, x_den, y_num, y_den), coefficients of x'^0, x'^1, ..."""
    x0, a, b = H2C_KERNEL_X, H2C_A, H2C_B
    x0sq = m.f2_sqr(x0)
    # x0 is a root of the 3-division polynomial 3 x^4 + 6 a x^2 + 12 b x - a^2
    psi3 = m.f2_sub(m.f2_add(m.f2_add(m.f2_muls(m.f2_sqr(x0sq), 3), m.f2_muls(m.f2_mul(a, x0sq), 6)), m.f2_muls(m.f2_mul(b, x0), 12)), m.f2_sqr(a))
    assert psi3 == (0, 0)
    gx = m.f2_add(m.f2_muls(x0sq, 3), a)
    v = m.f2_muls(gx, 2)
    u = m.f2_muls(m.f2_add(m.f2_add(m.f2_mul(x0sq, x0), m.f2_mul(a, x0)), b), 4)          # (2 y0)^2
    w = m.f2_add(u, m.f2_mul(x0, v))
    assert m.f2_sub(a, m.f2_muls(v, 5)) == (0, 0)                                       # the image curve has a = 0
    b_img = m.f2_sub(b, m.f2_muls(w, 7))
    d = [m.f2_neg(x0), (1, 0)]                                                          # x - x0
    d2, d3 = _pmul(d, d), _pmul(_pmul(d, d), d)
    xn = _padd(_padd(_pmul([(0, 0), (1, 0)], d2), [m.f2_mul(v, c) for c in d]), [u])   # X = x + v / (x - x0) + u / (x - x0)^2
    yn = _padd(_padd(d3, [m.f2_neg(m.f2_mul(v, c)) for c in d]), [m.f2_neg(m.f2_muls(u, 2))])   # Y = y (1 - v / (x - x0)^2 - 2 u / (x - x0)^3)
    t = m.f2_mul(b_img, m.f2_inv((4, 4)))                                               # s^6
    c = f2_cbrt(t)
    s0 = f2_sqrt(c)
    assert s0 is not None and m.f2_pow(s0, 6) == t
    zeta = m.f2_neg(m.f2_pow((1, 1), (P * P - 1) // 3))                                 # a primitive sixth root of unity
    assert m.f2_pow(zeta, 6) == (1, 0) and m.f2_pow(zeta, 3) != (1, 0) and m.f2_pow(zeta, 2) != (1, 0)
    out, s = [], s0
    for _ in range(6):
        i2 = m.f2_inv(m.f2_sqr(s))
        i3 = m.f2_mul(i2, m.f2_inv(s))
        out.append(([m.f2_mul(c, i2) for c in xn], d2, [m.f2_mul(c, i3) for c in yn], d3))
        s = m.f2_mul(s, zeta)
    return out


# RFC 9380 appendix E.3, coefficients of x'^0, x'^1, ...: what the derivation below must arrive at
_K = 0x5c759507e8e333ebb5b7a9a47d7ed8532c52d39fd3a042a88b58423c50ae15d5c2638e343d9c71c6238aaaaaaaa97d6
_L = 0x1530477c7ab4113b59a4c18b076d11930f7da5d4a07f649bf54439d87d27e500fc8c25ebf8c92f6812cfc71c71c6d706
H2C_TABLE = (
    [(_K, _K),
     (0, 0x11560bf17baa99bc32126fced787c88f984f87adf7ae0c7f9a208c6b4f20a4181472aaa9cb8d555526a9ffffffffc71a),
     (0x11560bf17baa99bc32126fced787c88f984f87adf7ae0c7f9a208c6b4f20a4181472aaa9cb8d555526a9ffffffffc71e,
      0x8ab05f8bdd54cde190937e76bc3e447cc27c3d6fbd7063fcd104635a790520c0a395554e5c6aaaa9354ffffffffe38d),
     (0x171d6541fa38ccfaed6dea691f5fb614cb14b4e7f4e810aa22d6108f142b85757098e38d0f671c7188e2aaaaaaaa5ed1, 0)],
    [(0, P - 72), (12, P - 12), (1, 0)],
    [(_L, _L),
     (0, 0x5c759507e8e333ebb5b7a9a47d7ed8532c52d39fd3a042a88b58423c50ae15d5c2638e343d9c71c6238aaaaaaaa97be),
     (0x11560bf17baa99bc32126fced787c88f984f87adf7ae0c7f9a208c6b4f20a4181472aaa9cb8d555526a9ffffffffc71c,
      0x8ab05f8bdd54cde190937e76bc3e447cc27c3d6fbd7063fcd104635a790520c0a395554e5c6aaaa9354ffffffffe38f),
     (0x124c9ad43b6cf79bfbf7043de3811ad0761b0f37a1e26286b0e977c69aa274524e79097a56dc4bd9e1b371c71c718b10, 0)],
    [(P - 432, P - 432), (0, P - 216), (18, P - 18), (1, 0)],
)


def h2c_consts():
    """(name -> Fp2 constant of the hash-to-G2 kernels, the isogeny): of the six scalings exactly one is the suite's table"""
    cands = h2c_isogeny_candidates()
    assert len({tuple(c[0]) for c in cands}) == 3 and len({(tuple(c[0]), tuple(c[2])) for c in cands}) == 6
    hit = [c for c in cands if c == H2C_TABLE]
    assert len(hit) == 1, "exactly one scaling is the suite's table"
    iso = hit[0]
    xn, xd, yn, yd = iso
    assert m.f2_mul(m.f2_sqr(xn[3]), xn[3]) == m.f2_sqr(yn[3])
    out = {}
    for nm, coeffs in (("XNUM", xn), ("YNUM", yn)):
        for i, cf in enumerate(coeffs):
            out["ISO_%s%d" % (nm, i)] = cf
    out["ISO_DEN"] = m.f2_neg(H2C_KERNEL_X)                                             # x_den = (x + DEN)^2, y_den = (x + DEN)^3
    out["SSWU_A"], out["SSWU_B"], out["SSWU_Z"] = H2C_A, H2C_B, H2C_Z
    out["SSWU_NBA"] = m.f2_mul(m.f2_neg(H2C_B), m.f2_inv(H2C_A))                        # -B / A
    out["SSWU_X1E"] = m.f2_mul(H2C_B, m.f2_inv(m.f2_mul(H2C_Z, H2C_A)))                 # B / (Z A): x1 of the exceptional case
    z3 = m.f2_mul(m.f2_sqr(H2C_Z), H2C_Z)
    out["SSWU_Z3"] = z3
    nz3 = (z3[0] * z3[0] + z3[1] * z3[1]) % P
    assert pow(nz3, (P - 1) // 2, P) == P - 1                                           # Z is no square: neither is the norm of Z^3
    out["SSWU_C"] = (pow(nz3, (P + 1) // 4, P), 0)                                      # c^2 = -norm(Z^3)
    return out, iso


# ---------------------------------------------------------------------------------------------------- hash-to-G1 (RFC 9380, zkp_bls_minsig.hip)
# E1': y^2 = x^3 + A x + B, 11-isogenous to E: y^2 = x^3 + 4.  The isogeny's 53 coefficients are DERIVED: the kernel is the one rational
# subgroup of order 11, Velu's formulas give a map onto y^2 = x^3 + 4 * 11^6, and of the six scalings (x, y) -> (x / s^2, y / s^3) with
# s^6 = 11^6 exactly one (s = 11) reproduces the RFC's vectors (tests/golden/h2c_g1_vectors.json).
G1H_A = 0x00144698a3b8e9433d693a02c96d4982b0ea985383ee66a8d8e8981aefd881ac98936f8da0e0f97f5cf428082d584c1d
G1H_B = 0x12e2908d11688030018b12e8753eee3b2016c1f0f24f4070a0b9c14fcef35ef55a23215a316ceaa5d1cc48e98e172be0
G1H_Z = 11
G1H_ORDER = (m.BLS_X + 1) ** 2 // 3 * m.R_ORDER         # #E(Fp) = #E1'(Fp): the curves are isogenous
G1H_H_EFF = m.BLS_X + 1                                # 1 - x


def _e1_add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = (3 * x1 * x1 + G1H_A) * m.fp_inv(2 * y1 % P) % P
    else:
        lam = (y2 - y1) * m.fp_inv((x2 - x1) % P) % P
    x3 = (lam * lam - x1 - x2) % P
    return (x3, (lam * (x1 - x3) - y1) % P)


def _e1_mul(pt, k):
    r = None
    for bit in bin(k)[2:]:
        r = _e1_add(r, r)
        if bit == "1":
            r = _e1_add(r, pt)
    return r


def _e1_rhs(x):
    return (x * x * x + G1H_A * x + G1H_B) % P


def g1h_kernel():
    """T, 2 T, .., 5 T, T a generator of the rational 11-torsion of E1' (cyclic: 121 | #E1' but one subgroup of order 11 is rational)"""
    assert G1H_ORDER % 121 == 0
    x = 1
    while True:
        x += 1
        y = m.fp_sqrt(_e1_rhs(x))
        if y is None:
            continue
        assert _e1_mul((x, y), G1H_ORDER) is None                                       # E1' is isogenous to E
        t = _e1_mul((x, y), G1H_ORDER // 121)
        if t is None:
            continue
        while _e1_mul(t, 11) is not None:
            t = _e1_mul(t, 11)
        pts = [t]
        for _ in range(4):
            pts.append(_e1_add(pts[-1], t))
        assert _e1_add(_e1_add(pts[4], t), pts[4]) is None and len({q[0] for q in pts}) == 5
        return pts


def _qmul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % P
    return out


def _qadd(a, b):
    n = max(len(a), len(b))
    return [((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % P for i in range(n)]


def _qeval(c, x):
    acc = 0
    for k in reversed(c):
        acc = (acc * x + k) % P
    return acc


def g1h_velu():
    """Velu's isogeny of that kernel as (x_num, x_den, y_num, y_den), coefficients of x^0, x^1, ..: X = x_num / x_den,
    Y = y y_num / y_den with x_den = D^2, y_den = D^3, D = prod (x - x_Q); and the image curve's b"""
    pts = g1h_kernel()
    lin = [[(-q[0]) % P, 1] for q in pts]

    def others(skip, power):
        r = [1]
        for j, f in enumerate(lin):
            if j != skip:
                for _ in range(power):
                    r = _qmul(r, f)
        return r
    d = others(-1, 1)
    d2, d3 = _qmul(d, d), _qmul(_qmul(d, d), d)
    xn, yn = _qmul([0, 1], d2), d3
    sv = sw = 0
    for i, (xq, yq) in enumerate(pts):
        v, u = 2 * (3 * xq * xq + G1H_A) % P, 4 * yq * yq % P
        sv, sw = (sv + v) % P, (sw + u + xq * v) % P
        xn = _qadd(xn, _qmul(_qadd([v * c % P for c in lin[i]], [u]), others(i, 2)))   # v / (x - xq) + u / (x - xq)^2
        yn = _qadd(yn, [(-c) % P for c in _qmul(_qadd([v * c % P for c in lin[i]], [2 * u % P]), others(i, 3))])
    assert (G1H_A - 5 * sv) % P == 0                                                    # the image curve has a = 0 ...
    b_img = (G1H_B - 7 * sw) % P
    assert b_img == 4 * 11 ** 6 == 0x6c20a4                                             # ... and b = 4 * 11^6
    assert len(xn) == 12 and len(d2) == 11 and len(yn) == 16 and len(d3) == 16
    return xn, d2, yn, d3


def g1h_scalings():
    g = 2
    while pow(g, (P - 1) // 2, P) == 1 or pow(g, (P - 1) // 3, P) == 1:
        g += 1
    w = pow(g, (P - 1) // 6, P)                                                         # a primitive sixth root of unity
    return [11 * pow(w, k, P) % P for k in range(6)]


def g1h_point(msg, dst, iso):
    """hash_to_curve of the suite with the rational map `iso`: hashlib, straight formulas, the group law of the model"""
    import hashlib
    dp = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + (128).to_bytes(2, "big") + b"\x00" + dp).digest()
    bs = [hashlib.sha256(b0 + b"\x01" + dp).digest()]
    for i in range(2, 5):
        bs.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, bs[-1])) + bytes([i]) + dp).digest())
    stream = b"".join(bs)
    acc = None
    for u in (int.from_bytes(stream[64 * i:64 * i + 64], "big") % P for i in range(2)):
        zu2 = G1H_Z * u * u % P
        tv1 = (zu2 * zu2 + zu2) % P
        x = G1H_B * m.fp_inv(G1H_Z * G1H_A % P) % P if tv1 == 0 else (-G1H_B) * m.fp_inv(G1H_A) % P * (1 + m.fp_inv(tv1)) % P
        y = m.fp_sqrt(_e1_rhs(x))
        if y is None:
            x = zu2 * x % P
            y = m.fp_sqrt(_e1_rhs(x))
        if (y & 1) != (u & 1):
            y = P - y
        xn, xd, yn, yd = iso
        dx, dy = _qeval(xd, x), _qeval(yd, x)
        if dx and dy:
            acc = m.g1_add(acc, (_qeval(xn, x) * m.fp_inv(dx) % P, y * _qeval(yn, x) % P * m.fp_inv(dy) % P))
    return m.g1_mul(acc, G1H_H_EFF) if acc is not None else None


_G1H = None


def g1h_consts():
    """(name -> Fp constant of the hash-to-G1 kernels, the isogeny as four coefficient lists): of the six scalings exactly one gives the
    suite's vectors"""
    global _G1H
    if _G1H is not None:
        return _G1H
    import json
    with open(os.path.join(ROOT, "tests", "golden", "h2c_g1_vectors.json")) as f:
        kat = json.load(f)
    xn, xd, yn, yd = g1h_velu()
    hit = []
    for s in g1h_scalings():
        i2 = m.fp_inv(s * s % P)
        i3 = i2 * m.fp_inv(s) % P
        iso = ([c * i2 % P for c in xn], xd, [c * i3 % P for c in yn], yd)
        if all(g1h_point(v["msg"].encode(), kat["dst"].encode(), iso) == tuple(int(c, 16) for c in v["p"]) for v in kat["vectors"]):
            hit.append((s, iso))
    assert len(hit) == 1 and hit[0][0] == 11, "exactly one scaling reproduces the vectors: s = 11"
    iso = hit[0][1]
    out = {"G1SSWU_A": G1H_A, "G1SSWU_B": G1H_B, "G1SSWU_Z": G1H_Z}
    c2 = m.fp_sqrt(P - G1H_Z)
    assert c2 is not None                                                               # sqrt_ratio's c2 = sqrt(-Z)
    out["G1SSWU_C2"] = c2
    for nm, coeffs in zip(("XNUM", "XDEN", "YNUM", "YDEN"), iso):
        for i, cf in enumerate(coeffs):
            out["G1ISO_%s%d" % (nm, i)] = cf
    _G1H = (out, iso)
    return _G1H


def balanced28(v):
    """14 signed limbs in [-2^27, 2^27) with sum l_i 2^(28 i) == v (v >= 0, v < 2^391)."""
    out = []
    carry = 0
    for i in range(14):
        d = ((v >> (28 * i)) & ((1 << 28) - 1)) + carry
        if i < 13 and d >= (1 << 27):
            d -= 1 << 28
            carry = 1
        else:
            carry = 0
        out.append(d)
    assert sum(l << (28 * i) for i, l in enumerate(out)) == v
    return out


def emit28(c):
    """28-bit-limb constants for the lane-cooperative family: Montgomery radix R = 2^392."""
    R392 = (1 << 392) % P

    def m28(v):
        return v * R392 % P

    names = [("ONE", R392), ("R2", R392 * R392 % P), ("R3", pow(R392, 3, P)), ("B", m28(4)), ("BETA", m28(c["BETA"]))]
    for k in ("G1_X", "G1_Y", "G2_X0", "G2_X1", "G2_Y0", "G2_Y1", "PSI_X_0", "PSI_X_1", "PSI_Y_0", "PSI_Y_1"):
        names.append((k, m28(c[k])))
    for i in range(1, 6):
        names.append(("GAMMA%d_0" % i, m28(c["GAMMA%d_0" % i])))
        names.append(("GAMMA%d_1" % i, m28(c["GAMMA%d_1" % i])))
    # hash-to-G2: 1 / 2, 2^256 R (the high half of a 512-bit value), p in balanced limbs, then the Fp2 constants
    names += [("INV2", m28((P + 1) // 2)), ("W256R", m28(m28(1 << 256)))]
    names.append(("PBAL", P))                                  # p itself (no Montgomery form) in balanced limbs: k_h2c_clear's renormalisation
    for k, v in h2c_consts()[0].items():
        names.append((k + "_0", m28(v[0])))
        names.append((k + "_1", m28(v[1])))
    pinv = (-pow(P, -1, 1 << 28)) % (1 << 28)
    lines = ["/* GENERATED by tools/gen_constants.py - do not edit.",
             " * 14 x 28-bit limbs.  ZKP28_P: unsigned limbs of p.  Everything in ZKP28_CONST_LIST is in Montgomery form",
             " * with R = 2^392 and BALANCED signed limbs in [-2^27, 2^27). */",
             "#pragma once", "#include <stdint.h>",
             "#define ZKP28_PINV 0x%07xu" % pinv,
             "#define ZKP28_P_LIMBS %s" % ", ".join("0x%07x" % x for x in limbs(P, 28, 14)),
             "/* divstep inversion (zkp_coop.hip f_inv): p in 13 limbs of 30 bits and p^-1 mod 2^30 */",
             "#define ZKP30_P_LIMBS %s" % ", ".join(str(x) for x in limbs(P, 30, 13)),
             "#define ZKP30_PINV %du" % pow(P, -1, 1 << 30),
             "#define ZKP28_CONST_LIST(X) \\"]
    for i, (k, v) in enumerate(names):
        lines.append("  X(%s, %s)%s" % (k, ", ".join(str(x) for x in balanced28(v)), " \\" if i + 1 < len(names) else ""))
    # hash-to-G1 (zkp_bls_minsig.hip): a list of its own, so that every line above stays as it was; the isogeny's 55 rows are in the order
    # x_num (12), x_den (11), y_num (16), y_den (16), each from x^0 up
    g1h = list(g1h_consts()[0].items())
    lines += ["/* hash-to-G1: simplified SWU on E1' and the 11-isogeny to E, same form as above */", "#define ZKP28_G1H_CONST_LIST(X) \\"]
    for i, (k, v) in enumerate(g1h):
        lines.append("  X(%s, %s)%s" % (k, ", ".join(str(x) for x in balanced28(m28(v))), " \\" if i + 1 < len(g1h) else ""))
    with open(os.path.join(ROOT, "zkvm_pairings_amd", "csrc", "zkp_constants28.h"), "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    c = consts()
    inv64 = (-pow(P, -1, 1 << 64)) % (1 << 64)
    inv32 = (-pow(P, -1, 1 << 32)) % (1 << 32)
    assert inv64 == 0x89F3FFFCFFFCFFFD  # matches reference src/common.rs:147

    lines = ["/* GENERATED by tools/gen_constants.py - do not edit. Montgomery form, R = 2^384, 6 x u64 LE. */",
             "#ifndef ORC_CONSTANTS_H", "#define ORC_CONSTANTS_H", "#include <stdint.h>",
             "#define ORC_INV64 0x%016xULL" % inv64,
             "#define ORC_BLS_X 0x%016xULL" % m.BLS_X,
             "static const uint64_t ORC_P[6] = %s;" % c_arr64(P),
             "static const uint64_t ORC_R_ORDER[4] = {%s};" % ", ".join("0x%016xULL" % x for x in limbs(m.R_ORDER, 64, 4)),
             "static const uint64_t ORC_P_MINUS_2[6] = %s;" % c_arr64(P - 2),
             "static const uint64_t ORC_P_PLUS_1_DIV_4[6] = %s;" % c_arr64((P + 1) // 4),
             "static const uint64_t ORC_P_MINUS_3_DIV_4[6] = %s;" % c_arr64((P - 3) // 4),
             "static const uint64_t ORC_P_MINUS_1_DIV_2[6] = %s;" % c_arr64((P - 1) // 2)]
    for k, v in c.items():
        if k == "P":
            continue
        if k in ("R", "R2"):
            lines.append("static const uint64_t ORC_%s[6] = %s;" % (k, c_arr64(v)))
        else:
            lines.append("static const uint64_t ORC_M_%s[6] = %s; /* mont(%s) */" % (k, c_arr64(mont(v)), k))
    # the same constants as plain integers, for the slow-mode build of the oracle (-DORC_SLOW: no Montgomery form)
    lines.append("#ifdef ORC_SLOW")
    for k, v in c.items():
        if k not in ("P", "R", "R2"):
            lines.append("static const uint64_t ORC_C_%s[6] = %s;" % (k, c_arr64(v)))
    lines.append("#endif")
    lines.append("#endif")
    with open(os.path.join(ROOT, "oracle", "orc_constants.h"), "w") as f:
        f.write("\n".join(lines) + "\n")

    lines = ["/* GENERATED by tools/gen_constants.py - do not edit. Montgomery form, R = 2^384, 12 x u32 LE. */",
             "#pragma once", "#include <stdint.h>",
             "#define ZKP_INV32 0x%08xu" % inv32,
             "#define ZKP_BLS_X 0x%016xULL" % m.BLS_X,
             "#define ZKP_CONST_LIST(X) \\"]
    names = []
    tbl = {"P": P, "R": c["R"], "R2": c["R2"], "P_MINUS_2": P - 2}
    for k, v in tbl.items():
        names.append((k, v))
    for k, v in c.items():
        if k in ("P", "R", "R2"):
            continue
        names.append(("M_" + k, mont(v)))
    for k, v in h2c_consts()[0].items():                      # hash-to-G2 (only these two headers: the oracle has no such map)
        names.append(("M_" + k + "_0", mont(v[0])))
        names.append(("M_" + k + "_1", mont(v[1])))
    for i, (k, v) in enumerate(names):
        lines.append("  X(%s, %s)%s" % (k, ", ".join("0x%08xu" % x for x in limbs(v, 32, 12)), " \\" if i + 1 < len(names) else ""))
    g1h = list(g1h_consts()[0].items())                       # hash-to-G1, a list of its own below the first
    lines.append("#define ZKP_G1H_CONST_LIST(X) \\")
    for i, (k, v) in enumerate(g1h):
        lines.append("  X(M_%s, %s)%s" % (k, ", ".join("0x%08xu" % x for x in limbs(mont(v), 32, 12)), " \\" if i + 1 < len(g1h) else ""))
    with open(os.path.join(ROOT, "zkvm_pairings_amd", "csrc", "zkp_constants.h"), "w") as f:
        f.write("\n".join(lines) + "\n")
    emit28(c)
    print("wrote oracle/orc_constants.h, zkvm_pairings_amd/csrc/zkp_constants.h and zkp_constants28.h")


if __name__ == "__main__":
    main()
