"""Python model of the compressed BLS12-381 point format (48 B per G1 point, 96 B per G2 point), on the integers of
golden/bls12_381_model.py.  It is the checker of zkp_g*_(de)compress_batch: nothing here calls the library.

Flags (top three bits of byte 0): 0x80 compressed, 0x40 infinity, 0x20 sort = y is the lexicographically larger of y and -y.
Decode statuses are zkp_point_status: 0 ok, 1 x >= p, 2 malformed, 3 no square root (not on the curve)."""
import bls12_381_model as m

P = m.P
HALF = (P - 1) // 2


def fp_sqrt(a):
    return m.fp_sqrt(a % P)


def fp2_sqrt_fast(a):
    """any square root of a = (a0, a1) in Fp2, or None: two Fp exponentiations and no inversion (the device's route)"""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        s = fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = fp_sqrt(-a0 % P)
        return None if s is None else (0, s)
    n = (a0 * a0 + a1 * a1) % P
    s = pow(n, (P + 1) // 4, P)
    if s * s % P != n:
        return None
    t = (a0 + s) * pow(2, -1, P) % P
    e = pow(t, (P - 3) // 4, P)
    c = t * e % P
    h = a1 * e * pow(2, -1, P) % P
    if c * c % P == t:
        return (c, h)
    return (-h % P, c)


def fp_is_big(y):
    return y > HALF


def fp2_is_big(y):
    return fp_is_big(y[1]) if y[1] else fp_is_big(y[0])


def _be(v):
    return v.to_bytes(48, "big")


def g1_compress(pt):
    """pt = (x, y) or None (infinity) -> 48 bytes"""
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    b = bytearray(_be(pt[0]))
    b[0] |= 0x80 | (0x20 if fp_is_big(pt[1]) else 0)
    return bytes(b)


def g2_compress(pt):
    """pt = ((x0, x1), (y0, y1)) or None -> 96 bytes (x.c1 first)"""
    if pt is None:
        return bytes([0xC0]) + bytes(95)
    (x0, x1), y = pt
    b = bytearray(_be(x1) + _be(x0))
    b[0] |= 0x80 | (0x20 if fp2_is_big(y) else 0)
    return bytes(b)


def _flags(b):
    """-> (status or None, infinity, sort)"""
    f = b[0] & 0xE0
    if not f & 0x80:
        return 2, False, False
    rest = bytes([b[0] & 0x1F]) + bytes(b[1:])
    if f & 0x40:
        return (2 if (f & 0x20) or any(rest) else None), True, False
    return None, False, bool(f & 0x20)


def g1_decompress(b):
    """48 bytes -> (status, point or None): point (x, y), None for the identity or a rejected string"""
    st, inf, sort = _flags(b)
    if st is not None or inf:
        return (st or 0), None
    x = int.from_bytes(bytes([b[0] & 0x1F]) + bytes(b[1:48]), "big")
    if x >= P:
        return 1, None
    y = fp_sqrt((x * x * x + 4) % P)
    if y is None:
        return 3, None
    if fp_is_big(y) != sort:
        y = -y % P
    return 0, (x, y)


def g2_decompress(b):
    """96 bytes -> (status, point or None): point ((x0, x1), (y0, y1))"""
    st, inf, sort = _flags(b)
    if st is not None or inf:
        return (st or 0), None
    x1 = int.from_bytes(bytes([b[0] & 0x1F]) + bytes(b[1:48]), "big")
    x0 = int.from_bytes(bytes(b[48:96]), "big")
    if x0 >= P or x1 >= P:
        return 1, None
    x = (x0, x1)
    rhs = m.f2_add(m.f2_mul(m.f2_sqr(x), x), (4, 4))
    y = fp2_sqrt_fast(rhs)
    if y is None:
        return 3, None
    if y != (0, 0) and fp2_is_big(y) != sort:
        y = m.f2_neg(y)
    return 0, (x, y)
