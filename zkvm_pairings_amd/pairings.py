"""Host-side mirror of the reference crate's pairing API (the module that is EMPTY upstream:
/root/reference/src/pairings.rs, declared at src/lib.rs:12), backed by the GPU engine.

    pairing(&G1Affine, &G2Affine) -> Gt
    multi_miller_loop(&[(&G1Affine, &G2Affine)]) -> MillerLoopResult
    MillerLoopResult::final_exponentiation() -> Gt
    Gt::identity()

Names, argument meaning and the infinity convention follow the reference's types
(G1Affine{x,y,is_infinity} src/g1.rs:7-11, G2Affine src/g2.rs:8-12, Fp12::one src/fp12.rs:87).
Every call executes on the GPU through the C ABI; there is no host arithmetic here."""
import numpy as np

from . import synthetic
from .engine import PairingEngine

_default = None


def default_engine():
    global _default
    if _default is None:
        _default = PairingEngine(0)
    return _default


P_MODULUS = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB


def _fp_neg(v):
    return (P_MODULUS - v) % P_MODULUS   # Fp::neg: zero stays zero


def _limbs(v):
    return [(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


class G1Affine:
    """reference src/g1.rs:7-11; identity is (0, 1, infinity) (src/g1.rs:25-31)."""

    def __init__(self, x, y, is_infinity=False):
        self.x, self.y, self.is_infinity = int(x), int(y), bool(is_infinity)

    @classmethod
    def identity(cls):
        return cls(0, 1, True)

    @classmethod
    def generator(cls):
        return cls.from_array(synthetic.G1_GENERATOR)

    @classmethod
    def from_array(cls, a, inf=False):
        a = np.asarray(a, dtype=np.uint64).reshape(12)
        f = lambda r: sum(int(v) << (64 * i) for i, v in enumerate(r))
        return cls(f(a[:6]), f(a[6:]), inf)

    def to_array(self):
        return np.array(_limbs(self.x) + _limbs(self.y), dtype=np.uint64)

    def is_identity(self):
        return self.is_infinity

    def to_compressed(self, engine=None):
        """48 bytes: x big-endian with the compression flag, the sort flag of y (y > (p-1)/2), or 0xc0 and zeros for the identity"""
        return (engine or default_engine()).compress_points(self.to_array(), 1, [1 if self.is_infinity else 0])

    @classmethod
    def from_compressed(cls, data, engine=None):
        """48 compressed bytes -> G1Affine on the curve (the subgroup is not checked: is_valid does that); ValueError otherwise"""
        if len(data) != 48:
            raise ValueError("a compressed G1 point has 48 bytes")
        pts, inf, st = (engine or default_engine()).decompress_points(bytes(data), 1)
        if st[0]:
            raise ValueError("not a compressed G1 point: %s" % PairingEngine.POINT_STATUS[int(st[0])])
        return cls.from_array(pts[0], bool(inf[0]))

    def is_valid(self, engine=None):
        """Ok(()) / Err(String) of src/g1.rs:49-62 as None / message."""
        st = (engine or default_engine()).g1_is_valid(self.to_array(), [1 if self.is_infinity else 0])[0]
        return {0: None, 1: "Point is not on curve", 2: "Point is not torsion free"}[int(st)]

    def __mul__(self, k):
        if self.is_infinity:
            return G1Affine.identity()
        out, inf = default_engine().g1_mul(self.to_array(), synthetic.int_to_scalar(int(k) % synthetic.R_ORDER))
        return G1Affine.from_array(out[0], bool(inf[0]))

    def __neg__(self):
        """src/g1.rs:118-128, on the host: y -> -y, the flag kept (the identity's y = 1 becomes p - 1, as upstream)"""
        return G1Affine(self.x, _fp_neg(self.y), self.is_infinity)

    def __add__(self, o):
        """src/g1.rs:155-187 on the GPU; P + (-P) is the identity (upstream panics there)"""
        out, inf = default_engine().g1_add(self.to_array(), o.to_array(), [1 if self.is_infinity else 0], [1 if o.is_infinity else 0])
        return G1Affine.from_array(out[0], bool(inf[0]))

    def __sub__(self, o):
        return self + (-o)

    def double(self):
        return self + self

    def __eq__(self, o):  # src/g1.rs:13-17 compares coordinates only
        return self.x == o.x and self.y == o.y


class G2Affine:
    """reference src/g2.rs:8-12."""

    def __init__(self, x, y, is_infinity=False):
        self.x, self.y, self.is_infinity = (int(x[0]), int(x[1])), (int(y[0]), int(y[1])), bool(is_infinity)

    @classmethod
    def identity(cls):
        return cls((0, 0), (1, 0), True)

    @classmethod
    def generator(cls):
        return cls.from_array(synthetic.G2_GENERATOR)

    @classmethod
    def from_array(cls, a, inf=False):
        a = np.asarray(a, dtype=np.uint64).reshape(24)
        f = lambda r: sum(int(v) << (64 * i) for i, v in enumerate(r))
        return cls((f(a[0:6]), f(a[6:12])), (f(a[12:18]), f(a[18:24])), inf)

    def to_array(self):
        return np.array(_limbs(self.x[0]) + _limbs(self.x[1]) + _limbs(self.y[0]) + _limbs(self.y[1]), dtype=np.uint64)

    def is_identity(self):
        return self.is_infinity

    def to_compressed(self, engine=None):
        """96 bytes: x.c1 | x.c0 big-endian with the compression flag and the sort flag of y (c1 decides, c0 when c1 == 0)"""
        return (engine or default_engine()).compress_points(self.to_array(), 2, [1 if self.is_infinity else 0])

    @classmethod
    def from_compressed(cls, data, engine=None):
        """96 compressed bytes -> G2Affine on the curve (the subgroup is not checked: is_valid does that); ValueError otherwise"""
        if len(data) != 96:
            raise ValueError("a compressed G2 point has 96 bytes")
        pts, inf, st = (engine or default_engine()).decompress_points(bytes(data), 2)
        if st[0]:
            raise ValueError("not a compressed G2 point: %s" % PairingEngine.POINT_STATUS[int(st[0])])
        return cls.from_array(pts[0], bool(inf[0]))

    def is_valid(self, engine=None):
        st = (engine or default_engine()).g2_is_valid(self.to_array(), [1 if self.is_infinity else 0])[0]
        return {0: None, 1: "Point is not on curve", 2: "Point is not torsion free"}[int(st)]

    def __mul__(self, k):
        if self.is_infinity:
            return G2Affine.identity()
        out, inf = default_engine().g2_mul(self.to_array(), synthetic.int_to_scalar(int(k) % synthetic.R_ORDER))
        return G2Affine.from_array(out[0], bool(inf[0]))

    def __neg__(self):
        """src/g2.rs:173-183, on the host"""
        return G2Affine(self.x, (_fp_neg(self.y[0]), _fp_neg(self.y[1])), self.is_infinity)

    def __add__(self, o):
        """src/g2.rs:210-242 on the GPU; P + (-P) is the identity (upstream panics there)"""
        out, inf = default_engine().g2_add(self.to_array(), o.to_array(), [1 if self.is_infinity else 0], [1 if o.is_infinity else 0])
        return G2Affine.from_array(out[0], bool(inf[0]))

    def __sub__(self, o):
        return self + (-o)

    def double(self):
        return self + self

    def __eq__(self, o):
        return self.x == o.x and self.y == o.y


class Gt:
    """Newtype over Fp12 (72 canonical u64 limbs); identity == Fp12::one() (src/fp12.rs:87-89)."""

    def __init__(self, limbs):
        self.limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(72)

    @classmethod
    def identity(cls):
        return cls(PairingEngine.gt_identity())

    def __eq__(self, o):  # limb equality, src/fp12.rs:46-50
        return bool(np.array_equal(self.limbs, o.limbs))

    def is_identity(self):
        return self == Gt.identity()


class MillerLoopResult:
    def __init__(self, limbs):
        self.limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(72)

    def final_exponentiation(self, engine=None):
        return Gt((engine or default_engine()).final_exponentiation(self.limbs)[0])

    def __eq__(self, o):
        return bool(np.array_equal(self.limbs, o.limbs))


def multi_miller_loop(terms, engine=None):
    """terms: sequence of (G1Affine, G2Affine).  Pairs with an identity on either side contribute one."""
    e = engine or default_engine()
    terms = list(terms)
    if not terms:
        return MillerLoopResult(PairingEngine.gt_identity())
    g1 = np.stack([p.to_array() for p, _ in terms])
    g2 = np.stack([q.to_array() for _, q in terms])
    i1 = np.array([p.is_infinity for p, _ in terms], dtype=np.uint8)
    i2 = np.array([q.is_infinity for _, q in terms], dtype=np.uint8)
    return MillerLoopResult(e.multi_miller_loop(g1, g2, len(terms), i1, i2)[0])


def final_exponentiation(ml, engine=None):
    return ml.final_exponentiation(engine)


def pairing(p, q, engine=None):
    e = engine or default_engine()
    out = e.pairing(p.to_array(), q.to_array(), [1 if p.is_infinity else 0], [1 if q.is_infinity else 0])
    return Gt(out[0])


def msm(points, scalars, engine=None):
    """sum_i [k_i] P_i on the GPU (bucket method) for a sequence of G1Affine or of G2Affine points and integer scalars (full 256-bit
    integers, not reduced mod r).  An empty sum is the identity of G1."""
    points, scalars = list(points), [int(k) for k in scalars]
    if len(points) != len(scalars):
        raise ValueError("%d points, %d scalars" % (len(points), len(scalars)))
    g2 = bool(points) and isinstance(points[0], G2Affine)
    cls = G2Affine if g2 else G1Affine
    if not points:
        return cls.identity()
    if any(k < 0 or k >> 256 for k in scalars):
        raise ValueError("msm: scalars are integers in [0, 2^256)")
    if any(not isinstance(p, cls) for p in points):
        raise TypeError("msm: mixed G1 and G2 points")
    e = engine or default_engine()
    pts = np.stack([p.to_array() for p in points])
    inf = np.array([p.is_infinity for p in points], dtype=np.uint8)
    sc = np.stack([synthetic.int_to_scalar(k) for k in scalars])
    out, oi = (e.g2_msm if g2 else e.g1_msm)(pts, sc, 1, inf)
    return cls.from_array(out[0], bool(oi[0]))
