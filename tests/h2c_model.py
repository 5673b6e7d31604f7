"""Big-integer model of RFC 9380 BLS12381G2_XMD:SHA-256_SSWU_RO_ and of minimal-pubkey-size BLS signatures: hashlib, Python integers
and the group law of tests/golden/bls12_381_model.py.  It imports nothing from the library.  TEST INFRASTRUCTURE ONLY."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import bls12_381_model as m  # noqa: E402

P = m.P
R_ORDER = m.R_ORDER
X_ABS = m.BLS_X                      # the curve parameter is x = -X_ABS
ETH_DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
RFC_DST = b"QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_RO_"
L_BYTES = 64                         # ceil((381 + 128) / 8)

# E': y^2 = x^3 + A x + B, the curve 3-isogenous to E2: y^2 = x^3 + 4 (1 + i)
A_ISO = (0, 240)
B_ISO = (1012, 1012)
Z_SSWU = (P - 2, P - 1)              # -(2 + i)
KERNEL_X = (P - 6, 6)                # the abscissa of the isogeny's kernel: -6 + 6 i

H_EFF = 0xbc69f08f2ee75b3584c6a0ea91b352888e2a8e9145ad7689986ff031508ffe1329c2f178731db956d82bf015d1212b02ec0ec69d7477c1ae954cbc06689f6a359894c0adebbf6b4e8020005aaa95551

_C = 0x5c759507e8e333ebb5b7a9a47d7ed8532c52d39fd3a042a88b58423c50ae15d5c2638e343d9c71c6238aaaaaaaa97d6
_D = 0x1530477c7ab4113b59a4c18b076d11930f7da5d4a07f649bf54439d87d27e500fc8c25ebf8c92f6812cfc71c71c6d706
# coefficients of x'^0, x'^1, ...
ISO_XNUM = [
    (_C, _C),
    (0, 0x11560bf17baa99bc32126fced787c88f984f87adf7ae0c7f9a208c6b4f20a4181472aaa9cb8d555526a9ffffffffc71a),
    (0x11560bf17baa99bc32126fced787c88f984f87adf7ae0c7f9a208c6b4f20a4181472aaa9cb8d555526a9ffffffffc71e,
     0x8ab05f8bdd54cde190937e76bc3e447cc27c3d6fbd7063fcd104635a790520c0a395554e5c6aaaa9354ffffffffe38d),
    (0x171d6541fa38ccfaed6dea691f5fb614cb14b4e7f4e810aa22d6108f142b85757098e38d0f671c7188e2aaaaaaaa5ed1, 0),
]
ISO_XDEN = [(0, P - 72), (12, P - 12), (1, 0)]
ISO_YNUM = [
    (_D, _D),
    (0, 0x5c759507e8e333ebb5b7a9a47d7ed8532c52d39fd3a042a88b58423c50ae15d5c2638e343d9c71c6238aaaaaaaa97be),
    (0x11560bf17baa99bc32126fced787c88f984f87adf7ae0c7f9a208c6b4f20a4181472aaa9cb8d555526a9ffffffffc71c,
     0x8ab05f8bdd54cde190937e76bc3e447cc27c3d6fbd7063fcd104635a790520c0a395554e5c6aaaa9354ffffffffe38f),
    (0x124c9ad43b6cf79bfbf7043de3811ad0761b0f37a1e26286b0e977c69aa274524e79097a56dc4bd9e1b371c71c718b10, 0),
]
ISO_YDEN = [(P - 432, P - 432), (0, P - 216), (18, P - 18), (1, 0)]


# ------------------------------------------------------------------------------------------------ expand_message_xmd, hash_to_field
def expand_message_xmd(msg, dst, len_in_bytes):
    assert 0 < len(dst) <= 255
    ell = (len_in_bytes + 31) // 32
    assert ell <= 255 and len_in_bytes <= 65535
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + len_in_bytes.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    b = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(b)[:len_in_bytes]


def hash_to_field_g2(msg, dst):
    """(u0, u1), each an Fp2 element (c0, c1)"""
    u = expand_message_xmd(msg, dst, 4 * L_BYTES)
    e = [int.from_bytes(u[L_BYTES * i:L_BYTES * (i + 1)], "big") % P for i in range(4)]
    return (e[0], e[1]), (e[2], e[3])


# ------------------------------------------------------------------------------------------------ Fp2 helpers
def f2_is_square(a):
    n = (a[0] * a[0] + a[1] * a[1]) % P
    return n == 0 or pow(n, (P - 1) // 2, P) == 1


def f2_sqrt(a):
    """a square root of a, or None"""
    if a == (0, 0):
        return (0, 0)
    a0, a1 = a
    if a1 == 0:
        s = m.fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = m.fp_sqrt((-a0) % P)
        return None if s is None else (0, s)
    n = m.fp_sqrt((a0 * a0 + a1 * a1) % P)
    if n is None:
        return None
    inv2 = (P + 1) // 2
    t = (a0 + n) * inv2 % P
    c = m.fp_sqrt(t)
    if c is None:
        t = (a0 - n) * inv2 % P
        c = m.fp_sqrt(t)
        if c is None:
            return None
    r = (c, a1 * m.fp_inv(2 * c % P) % P)
    return r if m.f2_sqr(r) == a else None


def sgn0(a):
    return a[0] & 1 if a[0] else a[1] & 1


def _poly(coeffs, x):
    acc = (0, 0)
    for c in reversed(coeffs):
        acc = m.f2_add(m.f2_mul(acc, x), c)
    return acc


# ------------------------------------------------------------------------------------------------ the curve E' (a != 0)
def iso_on_curve(pt):
    x, y = pt
    return m.f2_sqr(y) == m.f2_add(m.f2_add(m.f2_mul(m.f2_sqr(x), x), m.f2_mul(A_ISO, x)), B_ISO)


def iso_add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if m.f2_add(y1, y2) == (0, 0):
            return None
        lam = m.f2_mul(m.f2_add(m.f2_muls(m.f2_sqr(x1), 3), A_ISO), m.f2_inv(m.f2_muls(y1, 2)))
    else:
        lam = m.f2_mul(m.f2_sub(y2, y1), m.f2_inv(m.f2_sub(x2, x1)))
    x3 = m.f2_sub(m.f2_sub(m.f2_sqr(lam), x1), x2)
    return (x3, m.f2_sub(m.f2_mul(lam, m.f2_sub(x1, x3)), y1))


def sswu(u):
    """simplified SWU on E' (RFC 9380 section 6.6.2); returns (point, g(x1) was a square)"""
    zu2 = m.f2_mul(Z_SSWU, m.f2_sqr(u))
    tv1 = m.f2_add(m.f2_sqr(zu2), zu2)
    if tv1 == (0, 0):
        x1 = m.f2_mul(B_ISO, m.f2_inv(m.f2_mul(Z_SSWU, A_ISO)))
    else:
        x1 = m.f2_mul(m.f2_mul(m.f2_neg(B_ISO), m.f2_inv(A_ISO)), m.f2_add((1, 0), m.f2_inv(tv1)))
    g = lambda x: m.f2_add(m.f2_add(m.f2_mul(m.f2_sqr(x), x), m.f2_mul(A_ISO, x)), B_ISO)
    gx1 = g(x1)
    square = f2_is_square(gx1)
    if square:
        x, y = x1, f2_sqrt(gx1)
    else:
        x = m.f2_mul(zu2, x1)
        y = f2_sqrt(g(x))
    assert y is not None
    if sgn0(u) != sgn0(y):
        y = m.f2_neg(y)
    return (x, y), square


def iso3(pt):
    """the 3-isogeny E' -> E2; its kernel (x' = -6 + 6 i) and the identity go to the identity"""
    if pt is None:
        return None
    x, y = pt
    xd, yd = _poly(ISO_XDEN, x), _poly(ISO_YDEN, x)
    if xd == (0, 0) or yd == (0, 0):
        return None
    return (m.f2_mul(_poly(ISO_XNUM, x), m.f2_inv(xd)), m.f2_mul(y, m.f2_mul(_poly(ISO_YNUM, x), m.f2_inv(yd))))


# ------------------------------------------------------------------------------------------------ E2
def clear_cofactor_h_eff(pt):
    return m.g2_mul(pt, H_EFF)


def g2_mul_x(pt):
    """[x] P with the (negative) curve parameter"""
    return m.g2_neg(m.g2_mul(pt, X_ABS))


def clear_cofactor_psi(pt):
    """[x^2 - x - 1] P + [x - 1] psi(P) + psi^2(2 P)"""
    if pt is None:
        return None
    a = g2_mul_x(pt)                                     # x P
    psi_p = m.g2_psi(pt)
    b = m.g2_add(a, psi_p)                               # x P + psi(P)
    c = g2_mul_x(b) if b is not None else None           # x^2 P + x psi(P)
    dbl = m.g2_add(pt, pt)
    psi2 = m.g2_psi(m.g2_psi(dbl)) if dbl is not None else None
    out = m.g2_add(c, m.g2_neg(a))
    out = m.g2_add(out, m.g2_neg(pt))
    out = m.g2_add(out, m.g2_neg(psi_p))
    return m.g2_add(out, psi2)


LADDER_ADDS = (2, 12, 104, 53760, 53761 << 32)         # the multiple of the base the MSB-first ladder on X_ABS holds at its additions after the first


def _traced_add(p1, p2, site, seen):
    """p1 + p2 with the case csrc/zkp_bls_clear.hip's jac_add takes, tested in its order: the accumulator p1 at infinity, the operand p2 at
    infinity, equal points (doubled), opposite points, the generic formula"""
    if p1 is None:
        branch = "p_inf"
    elif p2 is None:
        branch = "q_inf"
    elif p1 == p2:
        branch = "dbl"
    elif p1 == m.g2_neg(p2):
        branch = "cancel"
    else:
        branch = "generic"
    seen.add((site, branch))
    return m.g2_add(p1, p2)


def _traced_ladder(base, site, seen):
    """[X_ABS] base as k_h2c_clear walks it: from the identity, MSB first, a doubling per bit and an addition per set bit"""
    r = None
    for b in range(63, -1, -1):
        r = m.g2_add(r, r)
        if (X_ABS >> b) & 1:
            r = _traced_add(r, base, site, seen)
    return r


def clear_cofactor_trace(pt):
    """clear_cofactor_psi in k_h2c_clear's order of operations: A = [|x|] P (site "A"), B = psi(P) + (-A) ("B"), C = [|x|] B ("C"),
    -C + A - P - psi(P) + psi^2(2 P) ("F0" .. "F3").  Returns (result, the set of (site, branch) its additions took)"""
    seen = set()
    a = _traced_ladder(pt, "A", seen)
    psi_p = m.g2_psi(pt) if pt is not None else None
    b = _traced_add(psi_p, m.g2_neg(a), "B", seen)
    c = _traced_ladder(b, "C", seen)
    dbl = m.g2_add(pt, pt)
    psi2 = m.g2_psi(m.g2_psi(dbl)) if dbl is not None else None
    r = m.g2_neg(c)
    for step, q in enumerate((a, m.g2_neg(pt), m.g2_neg(psi_p), psi2)):
        r = _traced_add(r, q, "F%d" % step, seen)
    return r, seen


def map_from_fields(u0, u1):
    q0, q1 = iso3(sswu(u0)[0]), iso3(sswu(u1)[0])
    return clear_cofactor_psi(m.g2_add(q0, q1))


def hash_to_g2(msg, dst):
    return map_from_fields(*hash_to_field_g2(msg, dst))


# ------------------------------------------------------------------------------------------------ signatures (public keys in G1)
def sk_to_pk(sk):
    return m.g1_mul(m.G1_GEN, sk % R_ORDER)


def sign(sk, msg, dst):
    return m.g2_mul(hash_to_g2(msg, dst), sk % R_ORDER)


def verify(pk, msg, sig, dst):
    """e(pk, H(m)) == e(g1, sig), points assumed valid"""
    if pk is None:
        return False
    if sig is None:
        return False
    lhs = m.pairing(pk, hash_to_g2(msg, dst))
    rhs = m.pairing(m.G1_GEN, sig)
    return lhs == rhs


# ------------------------------------------------------------------------------------------------ wire helpers (6 x u64 little-endian)
def fp_words(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def f2_words(a):
    return fp_words(a[0]) + fp_words(a[1])


def g2_words(pt):
    """(24 words, inf byte); the identity is (0, 1) with inf = 1, as the library writes it"""
    if pt is None:
        return [0] * 12 + [1] + [0] * 11, 1
    return f2_words(pt[0]) + f2_words(pt[1]), 0


def g1_words(pt):
    if pt is None:
        return [0] * 6 + [1] + [0] * 5, 1
    return fp_words(pt[0]) + fp_words(pt[1]), 0


def words_fp(w):
    return sum(int(x) << (64 * i) for i, x in enumerate(w))


def words_g2(w, inf):
    if inf:
        return None
    return ((words_fp(w[0:6]), words_fp(w[6:12])), (words_fp(w[12:18]), words_fp(w[18:24])))
