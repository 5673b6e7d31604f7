"""Field elements that reach the rare branches of the map to G2 (helper of test_h2c_cpu.py and test_gpu_h2c.py; not a test module), made
from fixed seeds on the integers of tests/h2c_model.py - nothing from the library under test.

Simplified SWU sends u to x1(u) = c (1 + 1 / (w^2 + w)) with w = Z u^2 and c = -B / A, and takes x2 = w x1 when g(x1) is no square.
  * w' = -1 - w has the same w^2 + w: whenever t' = -1 / Z - u^2 is a square, its roots +-u' share x1(u) with u, and on the x1 branch the
    two images have one abscissa; sgn0 decides whether the ordinates are equal or opposite, and u', -u' give one of each.
  * every abscissa x has preimages under x1: w^2 + w = 1 / (x / c - 1), a quadratic in w with discriminant 1 + 4 / (x / c - 1), then
    u = sqrt(w / Z) (about a quarter of all x have one).  With x = x2(u0) of a u0 on the x2 branch this gives a u1 on the x1 branch with the
    image of u0 or its negative: the same point, reached along two different computations.
  * g(x) lies in Fp iff 3 x_1 x_0^2 + 240 x_0 + (1012 - x_1^3) = 0 for x = x_0 + x_1 i (the imaginary part of x^3 + 240 i x + 1012 (1 + i)):
    a quadratic in x_0 for a chosen x_1.  Such a g(x) is always a square of Fp2; its root is real when g(x) is a residue of Fp and purely
    imaginary when it is not, and the kernel's square root takes another path for each (f2_sqrt_with_norm of csrc/zkp_bls.hip: p = 3 mod 4,
    so the root s of the norm g^2 is the residue among +-g, and t = (g + s) / 2 is g or zero).
The sum of the two mapped points then meets H = 0 in k_h2c_clear's first addition with operands that were not computed from one u.
TEST INFRASTRUCTURE ONLY."""
import bls12_381_model as m
import h2c_model as h
import replay_cases as rc

P = h.P
C_X = m.f2_mul(m.f2_neg(h.B_ISO), m.f2_inv(h.A_ISO))             # -B / A
COLLIDE_SEED, REAL_SEED, PARTNER_SEED = 0xC011, 0x9EA1, 0xADD
MAX_DRAWS = 200


def g_iso(x):
    return m.f2_add(m.f2_add(m.f2_mul(m.f2_sqr(x), x), m.f2_mul(h.A_ISO, x)), h.B_ISO)


def x1_of(u):
    """the first candidate abscissa of simplified SWU (u outside the exceptional case)"""
    w = m.f2_mul(h.Z_SSWU, m.f2_sqr(u))
    return m.f2_mul(C_X, m.f2_add((1, 0), m.f2_inv(m.f2_add(m.f2_sqr(w), w))))


def twin_square(u):
    """t' = -1 / Z - u^2: the other square with the same x1"""
    return m.f2_sub(m.f2_neg(m.f2_inv(h.Z_SSWU)), m.f2_sqr(u))


def roots_of_abscissa(x):
    """every u with x1(u) = x, as one root per sign pair (0, 1 or 2 of them)"""
    e = m.f2_sub(m.f2_mul(x, m.f2_inv(C_X)), (1, 0))
    if e == (0, 0):
        return []
    s = h.f2_sqrt(m.f2_add((1, 0), m.f2_muls(m.f2_inv(e), 4)))
    if s is None:
        return []
    inv2 = ((P + 1) // 2, 0)
    out = []
    for root in (s, m.f2_neg(s)):
        w = m.f2_mul(m.f2_sub(root, (1, 0)), inv2)
        u = h.f2_sqrt(m.f2_mul(w, m.f2_inv(h.Z_SSWU)))
        if u is not None and u != (0, 0) and u not in out and m.f2_neg(u) not in out:
            out.append(u)
    return out


def _draw(g):
    return (g.below(P), g.below(P))


def colliding_pairs():
    """{"same" | "opposite" | "cross_same" | "cross_opposite": [(u0, u1)]}, at least two of each, u1 not in {u0, -u0}: both on the x1
    branch with one image / opposite images; u0 on the x2 branch and u1 on the x1 branch with one image / opposite images"""
    def build():
        g = m.SplitMix64(COLLIDE_SEED)
        out = dict(same=[], opposite=[], cross_same=[], cross_opposite=[])
        for _ in range(MAX_DRAWS):
            if all(len(v) >= 2 for v in out.values()):
                break
            u0 = _draw(g)
            pt0, square = h.sswu(u0)
            if square:
                r, kind = h.f2_sqrt(twin_square(u0)), ""
            else:
                roots = roots_of_abscissa(pt0[0])
                r, kind = (roots[0] if roots else None), "cross_"
            if r is None or len(out[kind + "same"]) >= 2:
                continue
            for u1 in (r, m.f2_neg(r)):
                pt1, _ = h.sswu(u1)
                out[kind + ("same" if pt1[1] == pt0[1] else "opposite")].append((u0, u1))
        return out
    return rc._cached(("h2c-colliding",), build)


def real_g_elements(need=4):
    """{"residue" | "nonresidue": [u]}: `need` of each, g(x1(u)) in Fp and a residue / a non-residue there"""
    def build():
        g = m.SplitMix64(REAL_SEED)
        out = dict(residue=[], nonresidue=[])
        for _ in range(MAX_DRAWS):
            if all(len(v) >= need for v in out.values()):
                break
            xi = 1 + g.below(P - 1)
            s = m.fp_sqrt((240 * 240 - 12 * xi * (1012 - xi ** 3)) % P)
            if s is None:
                continue
            for root in (s, P - s):
                x = ((root - 240) * m.fp_inv(6 * xi % P) % P, xi)
                gx = g_iso(x)
                assert gx[1] == 0 and gx[0]
                kind = "residue" if pow(gx[0], (P - 1) // 2, P) == 1 else "nonresidue"
                for u in roots_of_abscissa(x)[:1]:
                    if len(out[kind]) < need:
                        out[kind].append(u)
        return out
    return rc._cached(("h2c-real-g", need), build)


def inputs():
    """[(label, u0, u1)]: every colliding pair in both orders, then every u with g(x1) in Fp next to a seeded partner, first and second in
    turn; one call of g2_map_from_fields takes them all"""
    rows = []
    for kind, pairs in colliding_pairs().items():
        for a, b in pairs:
            rows += [(kind, a, b), (kind + "-swapped", b, a)]
    g = m.SplitMix64(PARTNER_SEED)
    for kind, us in real_g_elements().items():
        for j, u in enumerate(us):
            other = _draw(g)
            rows.append((kind, u, other) if j % 2 == 0 else (kind + "-second", other, u))
    return rows


def expected():
    """the model's map of inputs(): [point or None]"""
    return rc._cached(("h2c-adversarial-expected",), lambda: [h.map_from_fields(a, b) for _, a, b in inputs()])


# ------------------------------------------------------------------------------------------------------------------- the cofactor chain
X = -h.X_ABS
H2 = (X ** 8 - 4 * X ** 7 + 5 * X ** 6 - 4 * X ** 4 + 6 * X ** 3 - 4 * X ** 2 - 4 * X + 13) // 9           # #E2 = H2 r
BIG_PRIME = 402096035359507321594726366720466575392706800671181159425656785868777272553337714697862511267018014931937703598282857976535744623203249
E2_FACTORS = {13: 2, 23: 2, 2713: 1, 11953: 1, 262069: 1, BIG_PRIME: 1, h.R_ORDER: 1}                           # prime -> exponent in #E2
E2_ORDER = H2 * h.R_ORDER
SMALL_ORDERS = (13, 23, 2713, 11953, 262069)
ORDER_SEED = 0x0DD
# Found by search among the first 40000 multiples of the generator (16 of them; these are the first four): at the addition "B" - for a
# point of G2 psi(P) = -A, so it doubles - the two sides of H = X2 Z1^2 - X1 Z2^2 come out of their Montgomery reductions as DIFFERENT
# integers of one residue class (a product lies in a window of length p that starts within p / 2^11 of zero, so this takes a value that
# close to zero).  H is then zero mod p with non-zero limbs: a kernel that tested the limbs alone would take the generic formula and
# return the identity.  The doubling is the one case where that matters: after a cancellation the generic formula's Z3 = 2 Z1 Z2 H is a
# product by a multiple of p, which the renormalisation brings to zero limbs anyway; and the two operands of the map's first addition,
# when they are one point, have gone through the same products and are the same integers (none of 19600 colliding pairs differed).
NEAR_ZERO_MULTIPLES = (3805, 6740, 8360, 12419)


def e2_point(g):
    return h.iso3(h.sswu(_draw(g))[0])


def point_of_order(ell):
    """a point of E2 of prime order ell: a seeded point times #E2 / ell^k, ell^k the whole power of ell in #E2 (the ell-part of E2 is not
    cyclic for 13 and 23: #E2 / ell would kill it)"""
    def build():
        g = m.SplitMix64(ORDER_SEED + ell)
        for _ in range(8):
            q = m.g2_mul(e2_point(g), E2_ORDER // ell ** E2_FACTORS[ell])
            if q is not None:
                assert m.g2_mul(q, ell) is None
                return q
        raise AssertionError("no point of order %d" % ell)
    return rc._cached(("h2c-order", ell), build)


def cofactor_points():
    """[(label, point or None)]: the inputs of the cofactor tests, chosen for the exceptional additions they take (test_h2c_cpu.py states
    which): the identity, points of G2 (NEAR_ZERO_MULTIPLES among them), seeded points of E2, the on-curve fixtures outside G2, every non-zero multiple of a point of order 13,
    a point of every other small prime order, and the sum of each of those with a point of G2"""
    def build():
        import outside_groups as og
        g = m.SplitMix64(ORDER_SEED)
        in_g2 = m.g2_mul(m.G2_GEN, 0xB0B)
        rows = [("identity", None), ("generator", m.G2_GEN), ("generator*2", m.g2_add(m.G2_GEN, m.G2_GEN)), ("generator*12345", m.g2_mul(m.G2_GEN, 12345)),
                ("generator*(r-1)", m.g2_neg(m.G2_GEN))]
        rows += [("generator*%d" % k, m.g2_mul(m.G2_GEN, k)) for k in NEAR_ZERO_MULTIPLES]
        rows += [("e2-%d" % j, e2_point(g)) for j in range(3)]
        rows += [("fixture-" + k, q) for k, q in og.g2_points().items() if m.g2_on_curve(q)]
        q13 = point_of_order(13)
        rows += [("order13*%d" % k, m.g2_mul(q13, k)) for k in range(1, 13)]
        small = [("order%d" % ell, point_of_order(ell)) for ell in SMALL_ORDERS[1:]]
        rows += small
        rows += [(name + "+g2", m.g2_add(q, in_g2)) for name, q in [("order13", q13)] + small]
        return rows
    return rc._cached(("h2c-cofactor-points",), build)


def cofactor_traces():
    """[(result, branches)] of h.clear_cofactor_trace on cofactor_points()"""
    return rc._cached(("h2c-cofactor-traces",), lambda: [h.clear_cofactor_trace(q) for _, q in cofactor_points()])
