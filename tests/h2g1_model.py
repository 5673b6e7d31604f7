"""Big-integer model of RFC 9380 BLS12381G1_XMD:SHA-256_SSWU_RO_ and of minimal-signature-size BLS signatures (signatures in G1, public
keys in G2): hashlib, Python integers and the group law of tests/golden/bls12_381_model.py.  The 11-isogeny is evaluated POINTWISE by
Velu's sums over a kernel found here - no coefficient list - so tools/gen_constants.py's rational functions have something independent
to agree with.  It imports nothing from the library.  TEST INFRASTRUCTURE ONLY."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import bls12_381_model as m  # noqa: E402
from h2c_model import expand_message_xmd, fp_words, g1_words, words_fp  # noqa: E402,F401

P = m.P
R_ORDER = m.R_ORDER
X_ABS = m.BLS_X
QUICKNET_DST = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"
RFC_DST = b"QUUX-V01-CS02-with-BLS12381G1_XMD:SHA-256_SSWU_RO_"
L_BYTES = 64

A_ISO = 0x00144698a3b8e9433d693a02c96d4982b0ea985383ee66a8d8e8981aefd881ac98936f8da0e0f97f5cf428082d584c1d
B_ISO = 0x12e2908d11688030018b12e8753eee3b2016c1f0f24f4070a0b9c14fcef35ef55a23215a316ceaa5d1cc48e98e172be0
Z_SSWU = 11
H_EFF = 0xd201000000010001                       # 1 - x
N_E = (X_ABS + 1) ** 2 // 3 * R_ORDER            # #E(Fp) = h r with h = (x - 1)^2 / 3
SCALE = 11                                       # the suite's map is (X / 11^2, Y / 11^3) after Velu


def hash_to_field_g1(msg, dst):
    u = expand_message_xmd(msg, dst, 2 * L_BYTES)
    return tuple(int.from_bytes(u[L_BYTES * i:L_BYTES * (i + 1)], "big") % P for i in range(2))


def sgn0(a):
    return a & 1


# ------------------------------------------------------------------------------------------------ a short Weierstrass curve over Fp
def ec_add(p1, p2, a):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = (3 * x1 * x1 + a) * m.fp_inv(2 * y1 % P) % P
    else:
        lam = (y2 - y1) * m.fp_inv((x2 - x1) % P) % P
    x3 = (lam * lam - x1 - x2) % P
    return (x3, (lam * (x1 - x3) - y1) % P)


def ec_mul(pt, k, a):
    r = None
    for b in bin(k)[2:] if k else "":
        r = ec_add(r, r, a)
        if b == "1":
            r = ec_add(r, pt, a)
    return r


def ec_neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % P)


def g_iso(x):
    return (x * x * x + A_ISO * x + B_ISO) % P


def iso_on_curve(pt):
    return pt[1] * pt[1] % P == g_iso(pt[0])


def e_on_curve(pt):
    return pt is None or pt[1] * pt[1] % P == (pt[0] ** 3 + 4) % P


def e_add(p1, p2):
    return ec_add(p1, p2, 0)


def e_mul(pt, k):
    return ec_mul(pt, k, 0)


def in_g1(pt):
    return e_on_curve(pt) and e_mul(pt, R_ORDER) is None


# ------------------------------------------------------------------------------------------------ the kernel of order 11 and Velu's sums
_KERNEL = None


def kernel_points():
    """T, 2 T, .., 5 T for a generator T of the one rational subgroup of order 11 of E1' (their negatives complete the kernel)"""
    global _KERNEL
    if _KERNEL is None:
        assert N_E % 121 == 0
        rng = random.Random(11)
        t = None
        while t is None:
            x = rng.randrange(P)
            y = m.fp_sqrt(g_iso(x))
            if y is None:
                continue
            t = ec_mul((x, y), N_E // 121, A_ISO)
            while t is not None and ec_mul(t, 11, A_ISO) is not None:
                t = ec_mul(t, 11, A_ISO)
        pts, q = [], t
        for _ in range(5):
            pts.append(q)
            q = ec_add(q, t, A_ISO)
        assert ec_add(q, pts[4], A_ISO) is None and len({p[0] for p in pts}) == 5
        _KERNEL = pts
    return _KERNEL


def velu(pt):
    """Velu's isogeny with the kernel above, unscaled: E1' -> y^2 = x^3 + 4 * 11^6; a kernel point goes to the identity"""
    if pt is None:
        return None
    x, y = pt
    big_x, dx = x, 1
    for (xq, yq) in kernel_points():
        d = (x - xq) % P
        if d == 0:
            return None
        v, u = 2 * (3 * xq * xq + A_ISO) % P, 4 * yq * yq % P
        i1 = m.fp_inv(d)
        i2 = i1 * i1 % P
        big_x = (big_x + v * i1 + u * i2) % P
        dx = (dx - v * i2 - 2 * u * i2 * i1) % P
    return (big_x, y * dx % P)


def iso11(pt, s=SCALE):
    q = velu(pt)
    if q is None:
        return None
    i = m.fp_inv(s)
    return (q[0] * i * i % P, q[1] * i * i * i % P)


def scalings():
    """the six s with s^6 = 11^6: 11 times the sixth roots of unity"""
    w = pow(2, (P - 1) // 6, P)
    g = 2
    while pow(w, 3, P) == 1 or pow(w, 2, P) == 1:
        g += 1
        w = pow(g, (P - 1) // 6, P)
    out = [11 * pow(w, k, P) % P for k in range(6)]
    assert len(set(out)) == 6 and all(pow(s, 6, P) == 11 ** 6 for s in out)
    return out


# ------------------------------------------------------------------------------------------------ simplified SWU (RFC 9380 6.6.2)
def sswu(u):
    """returns (point of E1', g(x1) was a square)"""
    zu2 = Z_SSWU * u * u % P
    tv1 = (zu2 * zu2 + zu2) % P
    if tv1 == 0:
        x1 = B_ISO * m.fp_inv(Z_SSWU * A_ISO % P) % P
    else:
        x1 = (-B_ISO) * m.fp_inv(A_ISO) % P * (1 + m.fp_inv(tv1)) % P
    gx1 = g_iso(x1)
    y = m.fp_sqrt(gx1)
    square = y is not None
    x = x1
    if not square:
        x = zu2 * x1 % P
        y = m.fp_sqrt(g_iso(x))
    assert y is not None
    if sgn0(u) != sgn0(y):
        y = (-y) % P
    return (x, y), square


def clear_cofactor(pt):
    return e_mul(pt, H_EFF)


def map_from_fields(u0, u1, s=SCALE):
    return clear_cofactor(e_add(iso11(sswu(u0)[0], s), iso11(sswu(u1)[0], s)))


def hash_to_g1(msg, dst, s=SCALE):
    return map_from_fields(*hash_to_field_g1(msg, dst), s=s)


# ------------------------------------------------------------------------------------------------ signatures (public keys in G2)
def sk_to_pk(sk):
    return m.g2_mul(m.G2_GEN, sk % R_ORDER)


def sign(sk, msg, dst):
    return e_mul(hash_to_g1(msg, dst), sk % R_ORDER)


def verify(pk, msg, sig, dst):
    """e(H(m), pk) == e(sig, g2), points assumed valid"""
    if pk is None or sig is None:
        return False
    return m.pairing(hash_to_g1(msg, dst), pk) == m.pairing(sig, m.G2_GEN)


def words_g1(w, inf):
    if inf:
        return None
    return (words_fp(w[0:6]), words_fp(w[6:12]))
