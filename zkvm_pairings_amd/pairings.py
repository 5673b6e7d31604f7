"""Host-side mirror of the reference crate's pairing API (the module that is EMPTY upstream:
/root/reference/src/pairings.rs, declared at src/lib.rs:12), backed by the GPU engine.

    pairing(&G1Affine, &G2Affine) -> Gt
    multi_miller_loop(&[(&G1Affine, &G2Affine)]) -> MillerLoopResult
    MillerLoopResult::final_exponentiation() -> Gt
    Gt::identity()

Names, argument meaning and the infinity convention follow the reference's types
(G1Affine{x,y,is_infinity} src/g1.rs:7-11, G2Affine src/g2.rs:8-12, Fp12::one src/fp12.rs:87).
Every call executes on the GPU through the C ABI; there is no host arithmetic here."""
import os

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


class Fr:
    """An element of the scalar field (reference src/fr.rs): a Python integer in [0, r).  Single elements are host integers - an
    operator on one element is not worth a launch; batches go through the engine (Fr.batch: zkp_fr_op_batch, Fr.fold: zkp_fr_fold_batch,
    Fr.from_bytes_wide: zkp_fr_from_wide_batch)."""
    MODULUS = synthetic.R_ORDER

    def __init__(self, v=0):
        self.v = int(v.v if isinstance(v, Fr) else v) % Fr.MODULUS

    @classmethod
    def from_array(cls, a):
        return cls(synthetic.scalar_to_int(np.asarray(a, dtype=np.uint64).reshape(4)))

    def to_array(self):
        return synthetic.int_to_scalar(self.v)

    def __int__(self):
        return self.v

    def __eq__(self, o):
        return self.v == Fr(o).v

    def __hash__(self):
        return hash(self.v)

    def __repr__(self):
        return "Fr(0x%064x)" % self.v

    def __add__(self, o):
        return Fr(self.v + Fr(o).v)

    def __sub__(self, o):
        return Fr(self.v - Fr(o).v)

    def __mul__(self, o):
        return Fr(self.v * Fr(o).v)

    def __neg__(self):
        return Fr(-self.v)

    def square(self):
        return Fr(self.v * self.v)

    def invert(self):
        """the inverse, or None for zero (src/fr.rs:266)"""
        return Fr(pow(self.v, Fr.MODULUS - 2, Fr.MODULUS)) if self.v else None

    @staticmethod
    def _rows(elems):
        elems = list(elems)
        return np.stack([Fr(e).to_array() for e in elems]) if elems else np.zeros((0, 4), dtype=np.uint64)

    @staticmethod
    def batch(op, a, b=None, engine=None):
        """[a_i op b_i] on the GPU; op: "mul", "add", "sub", "neg", "square", "invert" (0 inverts to 0)"""
        out = (engine or default_engine()).fr_op(op, Fr._rows(a), None if b is None else Fr._rows(b))
        return [Fr.from_array(r) for r in out]

    @staticmethod
    def fold(w, x, engine=None):
        """([sum_c w_c x_c[i] for i], sum_c w_c) on the GPU; x: one row of l elements per weight"""
        x = [list(row) for row in x]
        l = len(x[0]) if x else 0
        out, sw = (engine or default_engine()).fr_fold(Fr._rows(w), Fr._rows([e for row in x for e in row]), l)
        return [Fr.from_array(r) for r in out], Fr.from_array(sw)

    @staticmethod
    def invert_batch(a, engine=None):
        """[a_i^-1] on the GPU by Montgomery's trick (zkp_fr_invert_batch: one power per call); 0 inverts to 0"""
        return [Fr.from_array(r) for r in (engine or default_engine()).fr_invert(Fr._rows(a))]

    @staticmethod
    def evaluate(evals, z, bitrev=False, engine=None):
        """p(z) for the polynomial of degree < N with p(w^i) = evals[i] over the N-th roots of unity (N = len(evals), a power of two;
        evals[i] belongs to w^bitrev(i) with bitrev), on the GPU (zkp_fr_eval_batch)"""
        evals = list(evals)
        log2_n = len(evals).bit_length() - 1
        if len(evals) != 1 << log2_n:
            raise ValueError("the number of evaluations is not a power of two")
        out = (engine or default_engine()).fr_eval(Fr._rows(evals), Fr._rows([z]), log2_n, bitrev)
        return Fr.from_array(out[0])

    @staticmethod
    def ntt(coeffs, inverse=False, bitrev=False, coset=False, engine=None):
        """the evaluations of the polynomial sum_k coeffs[k] X^k over the N-th roots of unity w^i (N = len(coeffs), a power of two), on
        the GPU (zkp_fr_ntt_batch); coset: over 7 w^i; bitrev: slot i belongs to w^bitrev(i); inverse: evaluations in, coefficients out"""
        coeffs = list(coeffs)
        log2_n = len(coeffs).bit_length() - 1
        if len(coeffs) != 1 << log2_n:
            raise ValueError("the number of coefficients is not a power of two")
        out = (engine or default_engine()).fr_ntt(Fr._rows(coeffs), log2_n, inverse=inverse, bitrev=bitrev, coset=coset)
        return [Fr.from_array(r) for r in out]

    @staticmethod
    def from_bytes_wide(data, engine=None):
        """64 little-endian bytes -> the integer mod r (src/fr.rs:192-217), on the GPU"""
        if len(data) != 64:
            raise ValueError("from_bytes_wide takes 64 bytes")
        return Fr.from_array((engine or default_engine()).fr_from_wide(bytes(data))[0])


class Groth16VerifyingKey:
    """alpha in G1, beta / gamma / delta in G2 and IC_0 .. IC_l in G1 (l public inputs), as wire arrays; every point is finite"""

    def __init__(self, alpha_g1, beta_g2, gamma_g2, delta_g2, ic):
        arr = lambda p, w: (p.to_array() if hasattr(p, "to_array") else np.ascontiguousarray(p, dtype=np.uint64)).reshape(w)
        self.alpha_g1, self.beta_g2, self.gamma_g2, self.delta_g2 = arr(alpha_g1, 12), arr(beta_g2, 24), arr(gamma_g2, 24), arr(delta_g2, 24)
        ic = [arr(p, 12) for p in ic] if not isinstance(ic, np.ndarray) else ic
        self.ic = np.ascontiguousarray(ic, dtype=np.uint64).reshape(-1, 12)
        if self.ic.shape[0] < 1:
            raise ValueError("a verifying key holds at least IC_0")

    @property
    def n_inputs(self):
        return self.ic.shape[0] - 1

    def arrays(self):
        return self.alpha_g1, self.beta_g2, self.gamma_g2, self.delta_g2, self.ic


def _g2_neg_array(q):
    """-Q on a (24,) wire array, on the host like G2Affine.__neg__"""
    q = G2Affine.from_array(q)
    return (-q).to_array()


def _groth16_proofs(proofs, e):
    """(a, b, c, inf_a, inf_b, inf_c, decoded): proofs as three point arrays, or an (n, 192) uint8 array of compressed A | B | C
    (48 + 96 + 48 bytes) decompressed on the GPU from contiguous column copies; decoded[c] = 0 where a point of proof c failed to
    decompress"""
    if isinstance(proofs, (tuple, list)) and len(proofs) == 3:
        a, b, c = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, w) for x, w in zip(proofs, (12, 24, 12)))
        if not (a.shape[0] == b.shape[0] == c.shape[0]):
            raise ValueError("A, B and C differ in number of points")
        return a, b, c, None, None, None, np.ones(a.shape[0], dtype=bool)
    raw = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, 192)
    a, ia, sa = e.decompress_points(np.ascontiguousarray(raw[:, :48]), 1)
    b, ib, sb = e.decompress_points(np.ascontiguousarray(raw[:, 48:144]), 2)
    c, ic, sc = e.decompress_points(np.ascontiguousarray(raw[:, 144:]), 1)
    return a, b, c, ia, ib, ic, (sa | sb | sc) == 0


def _groth16_inputs(inputs, n, l):
    x = np.ascontiguousarray(inputs, dtype=np.uint64) if inputs is not None and l else np.zeros((n, 0, 4), dtype=np.uint64)
    if x.size != n * l * 4:
        raise ValueError("inputs hold %d elements for %d proofs of %d" % (x.size // 4, n, l))
    return x.reshape(n, l, 4)


def groth16_verify_batch(vk, proofs, inputs, engine=None, rand=None, points_checked=False, vk_checked=False):
    """True iff every one of the n proofs verifies against vk (zkp_groth16_verify_batch: one random combination, one final
    exponentiation; a batch with an invalid proof passes with probability <= 2^-128).  proofs: (A, B, C) point arrays or an (n, 192)
    uint8 array of compressed A | B | C - a proof that fails to decompress fails the batch; inputs (n, n_inputs, 4) uint64, each below
    r.  groth16_verify_each finds the bad proof when this returns False."""
    e = engine or default_engine()
    a, b, c, ia, ib, ic, decoded = _groth16_proofs(proofs, e)
    n = a.shape[0]
    x = _groth16_inputs(inputs, n, vk.n_inputs)
    if not decoded.all():
        return False
    return e.groth16_verify_batch(*vk.arrays(), a, b, c, x, inf_a=ia, inf_b=ib, inf_c=ic, rand=rand, points_checked=points_checked, vk_checked=vk_checked)


def groth16_verify_each(vk, proofs, inputs, engine=None):
    """bool array (n,): proof c verifies.  The per-proof path, composed only of calls that do not know Groth16: vk_x_c = IC_0 +
    sum_i x_{c,i} IC_{i+1} through msm(shared_bases) with the scalar 1 for IC_0, then pairing_check with k = 4 on
    (A_c, B_c), (alpha, -beta), (vk_x_c, -gamma), (C_c, -delta), ANDed with is_valid of every point and with every input < r."""
    e = engine or default_engine()
    a, b, c, ia, ib, ic, ok = _groth16_proofs(proofs, e)
    n, l = a.shape[0], vk.n_inputs
    x = _groth16_inputs(inputs, n, l)
    ok = ok.copy()
    if n == 0:
        return ok
    key_ok = not (e.g1_is_valid(vk.alpha_g1).any() or e.g1_is_valid(vk.ic).any() or
                  e.g2_is_valid(np.stack([vk.beta_g2, vk.gamma_g2, vk.delta_g2])).any())
    ok &= key_ok
    ok &= (e.g1_is_valid(a, ia) == 0) & (e.g2_is_valid(b, ib) == 0) & (e.g1_is_valid(c, ic) == 0)
    ok &= synthetic.below_r(x.reshape(-1, 4)).reshape(n, l).all(axis=1)
    sc = np.zeros((n, l + 1, 4), dtype=np.uint64)
    sc[:, 0, 0] = 1
    sc[:, 1:] = x
    vkx, vinf = np.empty((n, 12), dtype=np.uint64), np.empty(n, dtype=np.uint8)
    step = max(1, (1 << 24) // (l + 1))            # the MSM's limit on m * n_msm
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        vkx[lo:hi], vinf[lo:hi] = e.g1_msm(vk.ic, sc[lo:hi].reshape(-1, 4), hi - lo, shared_bases=True)
    g1 = np.empty((n, 4, 12), dtype=np.uint64)
    g2 = np.empty((n, 4, 24), dtype=np.uint64)
    g1[:, 0], g1[:, 1], g1[:, 2], g1[:, 3] = a, vk.alpha_g1, vkx, c
    g2[:, 0], g2[:, 1], g2[:, 2], g2[:, 3] = b, _g2_neg_array(vk.beta_g2), _g2_neg_array(vk.gamma_g2), _g2_neg_array(vk.delta_g2)
    i1 = np.zeros((n, 4), dtype=np.uint8)
    i2 = np.zeros((n, 4), dtype=np.uint8)
    i1[:, 2] = vinf
    if ia is not None:
        i1[:, 0], i2[:, 0], i1[:, 3] = ia, ib, ic
    per, _ = e.pairing_check(g1.reshape(-1, 12), g2.reshape(-1, 24), 4, i1.reshape(-1), i2.reshape(-1))
    return ok & (np.asarray(per).reshape(-1) != 0)


class R1CS:
    """A rank-one constraint system over the N = 2^log2_n-point domain: three sparse matrices A, B, C of n_rows x m in compressed rows,
    each a tuple (row_ptr (n_rows + 1) uint32, col (nnz) uint32, val (nnz, 4) uint64, canonical).  Variable 0 is the constant one,
    variables 1 .. n_inputs are public.  No input-consistency rows are added (include/zkp_prove.h)."""

    def __init__(self, log2_n, n_rows, m, n_inputs, a, b, c):
        self.log2_n, self.n_rows, self.m, self.n_inputs = int(log2_n), int(n_rows), int(m), int(n_inputs)
        if self.n_rows > 1 << self.log2_n or self.n_inputs + 1 > self.m:
            raise ValueError("more rows than the domain holds, or more public inputs than variables")
        mats = []
        for row_ptr, col, val in (a, b, c):
            mats.append((np.ascontiguousarray(row_ptr, dtype=np.uint32).reshape(-1), np.ascontiguousarray(col, dtype=np.uint32).reshape(-1),
                         np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)))
        self.a, self.b, self.c = mats

    def matrices(self):
        """the three matrices as the engine takes them: (n_rows, n_cols, row_ptr, col, val)"""
        return tuple((self.n_rows, self.m) + x for x in (self.a, self.b, self.c))


class Groth16ProvingKey:
    """A Groth16 proving key as wire arrays, the fields of zkp_groth16_pk: alpha_g1, beta_g1, delta_g1 (12,), beta_g2, delta_g2 (24,),
    a_query and b_g1_query (m, 12), b_g2_query (m, 24), l_query (m - n_inputs - 1, 12), h_query (N - 1, 12); a_inf, b_g1_inf, b_g2_inf,
    l_inf: optional infinity bytes of the four per-variable queries.  The points are trusted: check a key once with g1_is_valid /
    g2_is_valid."""
    FIELDS = tuple(name for name, _ in PairingEngine._PK_FIELDS)

    def __init__(self, **arrays):
        unknown = set(arrays) - set(self.FIELDS)
        if unknown:
            raise ValueError("unknown proving key fields: %s" % sorted(unknown))
        for name, w in PairingEngine._PK_FIELDS:
            x = arrays.get(name)
            if x is not None:
                x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1) if w is None else np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, w)
            setattr(self, name, x)

    def arrays(self):
        return {name: getattr(self, name) for name in self.FIELDS}


def groth16_quotient_batch(r1cs, witnesses, engine=None):
    """(h (n, N, 4), sat (n,)): the quotient polynomial h = (a b - c) / (X^N - 1) of each witness (n, m, 4) by its N coefficients, and
    whether the witness satisfies every constraint (zkp_groth16_quotient_batch)."""
    e = engine or default_engine()
    return e.groth16_quotient(r1cs.log2_n, r1cs.n_inputs, *r1cs.matrices(), witnesses)


def groth16_prove_batch(r1cs, pk, witnesses, rs=None, engine=None):
    """n proofs of one circuit on the GPU (zkp_groth16_prove_batch) -> ((A (n, 12), B (n, 24), C (n, 12)), (inf_a, inf_b, inf_c), sat):
    the proofs in the form groth16_verify_batch takes, and sat[j] = 1 iff witness j satisfies the system (the proof of an unsatisfied
    witness is written too; it does not verify).  rs (n, 2, 4): the blinding scalars r_j, s_j, by default fresh from os.urandom and
    reduced below r - never a seeded generator; zeros give a deterministic proof without zero knowledge."""
    e = engine or default_engine()
    w = np.ascontiguousarray(witnesses, dtype=np.uint64)
    n = w.size // (4 * r1cs.m) if r1cs.m else 0
    if rs is None:
        rs = e.fr_from_wide(np.frombuffer(os.urandom(n * 2 * 64), dtype=np.uint8).reshape(n * 2, 64)) if n else np.zeros((0, 8), dtype=np.uint64)
    pa, ia, pb, ib, pc, ic, sat = e.groth16_prove(r1cs.log2_n, r1cs.n_inputs, *r1cs.matrices(), pk.arrays(), w, rs)
    return (pa, pb, pc), (ia, ib, ic), sat


class KzgSetup:
    """the verifier's side of a KZG setup: g1 in G1, g2 and [tau] g2 in G2, as wire arrays; every point is finite"""

    def __init__(self, g1, g2, tau_g2):
        arr = lambda p, w: (p.to_array() if hasattr(p, "to_array") else np.ascontiguousarray(p, dtype=np.uint64)).reshape(w)
        self.g1, self.g2, self.tau_g2 = arr(g1, 12), arr(g2, 24), arr(tau_g2, 24)

    def arrays(self):
        return self.g1, self.g2, self.tau_g2


def _kzg_arrays(commitments, z, y, proofs):
    c, p = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 12) for x in (commitments, proofs))
    z, y = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in (z, y))
    if not (c.shape[0] == p.shape[0] == z.shape[0] == y.shape[0]):
        raise ValueError("commitments, z, y and proofs differ in number")
    return c, z, y, p


def kzg_verify_batch(setup, commitments, z, y, proofs, engine=None, rand=None, inf_c=None, inf_proof=None, points_checked=False, vk_checked=False):
    """True iff every one of the n openings (C_i, z_i, y_i, pi_i) holds against the setup (zkp_kzg_verify_batch: one random combination,
    one MSM call, one final exponentiation; a batch with a false opening passes with probability <= 2^-128).  commitments / proofs (n, 12),
    z / y (n, 4) uint64, each below r.  kzg_verify_each finds the bad opening when this returns False."""
    e = engine or default_engine()
    c, z, y, p = _kzg_arrays(commitments, z, y, proofs)
    return e.kzg_verify_batch(*setup.arrays(), c, z, y, p, inf_c=inf_c, inf_proof=inf_proof, rand=rand, points_checked=points_checked,
                              vk_checked=vk_checked)


def kzg_verify_each(setup, commitments, z, y, proofs, engine=None, inf_c=None, inf_proof=None):
    """bool array (n,): opening i holds.  The per-opening path, composed only of calls that do not know KZG: -[y_i] g1 + [z_i] pi_i
    through msm (n sums of two terms), C_i added by g1_add, then pairing_check with k = 2 on (C_i - [y_i] g1 + [z_i] pi_i, -g2),
    (pi_i, [tau] g2), ANDed with is_valid of every point and with z_i, y_i < r."""
    e = engine or default_engine()
    c, z, y, p = _kzg_arrays(commitments, z, y, proofs)
    n = c.shape[0]
    ok = np.ones(n, dtype=bool)
    if n == 0:
        return ok
    ic = np.zeros(n, dtype=np.uint8) if inf_c is None else np.ascontiguousarray(inf_c, dtype=np.uint8).reshape(n)
    ip = np.zeros(n, dtype=np.uint8) if inf_proof is None else np.ascontiguousarray(inf_proof, dtype=np.uint8).reshape(n)
    ok &= not (e.g1_is_valid(setup.g1).any() or e.g2_is_valid(np.stack([setup.g2, setup.tau_g2])).any())
    ok &= (e.g1_is_valid(c, ic) == 0) & (e.g1_is_valid(p, ip) == 0)
    ok &= synthetic.below_r(z) & synthetic.below_r(y)
    r = synthetic.R_ORDER
    pts = np.empty((n, 2, 12), dtype=np.uint64)
    pts[:, 0], pts[:, 1] = setup.g1, p
    sc = np.empty((n, 2, 4), dtype=np.uint64)
    sc[:, 0] = synthetic._rows([-v % r for v in synthetic._ints(y)])
    sc[:, 1] = z
    inf = np.zeros((n, 2), dtype=np.uint8)
    inf[:, 1] = ip
    s, s_inf = e.g1_msm(pts.reshape(-1, 12), sc.reshape(-1, 4), n, inf.reshape(-1))
    lhs, lhs_inf = e.g1_add(c, s, ic, s_inf)
    g1 = np.empty((n, 2, 12), dtype=np.uint64)
    g2 = np.empty((n, 2, 24), dtype=np.uint64)
    g1[:, 0], g1[:, 1] = lhs, p
    g2[:, 0], g2[:, 1] = _g2_neg_array(setup.g2), setup.tau_g2
    i1 = np.zeros((n, 2), dtype=np.uint8)
    i1[:, 0], i1[:, 1] = lhs_inf, ip
    per, _ = e.pairing_check(g1.reshape(-1, 12), g2.reshape(-1, 24), 2, i1.reshape(-1), np.zeros(2 * n, dtype=np.uint8))
    return ok & (np.asarray(per).reshape(-1) != 0)


def _kzg_poly_arrays(lagrange_g1, evals):
    setup = np.ascontiguousarray(lagrange_g1, dtype=np.uint64).reshape(-1, 12)
    big_n = setup.shape[0]
    log2_n = big_n.bit_length() - 1
    ev = np.ascontiguousarray(evals, dtype=np.uint64)
    if big_n < 1 or big_n != 1 << log2_n or ev.size % (4 * big_n):
        raise ValueError("%d setup points and %d evaluations: no whole number of polynomials of a power-of-two size" % (big_n, ev.size // 4))
    return setup, ev.reshape(-1, 4), log2_n, ev.size // (4 * big_n)


def kzg_commit_batch(lagrange_g1, evals, engine=None):
    """(commitments (n, 12), inf (n,)): C_j = sum_i evals[j][i] lagrange_g1[i] = [f_j(tau)] g1 for polynomials in evaluation form over the
    N = len(lagrange_g1) roots of unity, the setup in the same order as the evaluations (natural or bit-reversed): ONE shared-bases MSM
    (g1_msm) of n sums over the N setup points.  evals (n, N, 4)."""
    e = engine or default_engine()
    setup, ev, _, n = _kzg_poly_arrays(lagrange_g1, evals)
    if n == 0:
        return np.zeros((0, 12), dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    return e.g1_msm(setup, ev, n, None, shared_bases=True)


def kzg_open_batch(lagrange_g1, evals, z, bitrev=True, engine=None):
    """(y (n, 4), proofs (n, 12), inf (n,)): polynomial j - its N evaluations evals[j] over the N-th roots of unity, in bit-reversed order
    with bitrev as blobs are stored - opened at z[j] on the GPU (zkp_kzg_open_batch): y[j] = f_j(z[j]), proofs[j] = [q_j(tau)] g1 with
    q_j = (f_j - y[j]) / (X - z[j]).  lagrange_g1 (N, 12) is the setup in the order of the evaluations, trusted.  The result is what
    kzg_verify_batch consumes."""
    e = engine or default_engine()
    setup, ev, log2_n, n = _kzg_poly_arrays(lagrange_g1, evals)
    z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
    if z.shape[0] != n:
        raise ValueError("%d points for %d polynomials" % (z.shape[0], n))
    return e.kzg_open(setup, ev, z, log2_n, bitrev)


def _pow2_points(points, what):
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 12)
    big_n = pts.shape[0]
    log2_n = big_n.bit_length() - 1
    if big_n < 1 or big_n != 1 << log2_n:
        raise ValueError("%s: %d points is no power of two" % (what, big_n))
    return pts, log2_n


def g1_ntt(points, log2_n, inverse=False, bitrev=False, inf=None, engine=None):
    """(out (n, 12), out_inf (n,)): the number-theoretic transform of vectors of 2^log2_n G1 points each over the roots of unity of fr_ntt
    (zkp_g1_ntt_batch): out[j][i] = sum_k [w^(i k)] points[j][k]; inverse and bitrev as in fr_ntt.  The points are trusted."""
    return (engine or default_engine()).g1_ntt(points, log2_n, inverse=inverse, bitrev=bitrev, inf=inf)


class Fk20Setup:
    """What kzg_open_domain_batch needs of a setup: the 2N points (and their infinity flags) that zkp_kzg_fk20_setup derives from the
    monomial setup [tau^k] g1, k < N.  Build it once per setup with kzg_fk20_setup."""

    def __init__(self, points, inf, log2_n):
        self.points, self.inf, self.log2_n = points, inf, int(log2_n)

    @property
    def n(self):
        return 1 << self.log2_n


def kzg_fk20_setup(monomial_g1, engine=None):
    """Fk20Setup of the monomial setup monomial_g1 (N, 12), N a power of two (zkp_kzg_fk20_setup).  The points are trusted: check a
    ceremony's output once with g1_is_valid."""
    e = engine or default_engine()
    mono, log2_n = _pow2_points(monomial_g1, "kzg_fk20_setup")
    pts, inf = e.kzg_fk20_setup(mono, log2_n)
    return Fk20Setup(pts, inf, log2_n)


def kzg_open_domain_batch(setup, coeffs, bitrev=True, engine=None):
    """(proofs (n, N, 12), inf (n, N)): polynomial j, given by its N coefficients coeffs[j], opened at EVERY N-th root of unity by the
    Feist-Khovratovich method (zkp_kzg_fk20_batch): proofs[j][m] = [(f_j(tau) - f_j(w^m)) / (tau - w^m)] g1, slot m belonging to
    w^bitrev(m) with bitrev, as blobs are stored.  The opened values are fr_ntt(coeffs, bitrev=bitrev).  setup: an Fk20Setup."""
    e = engine or default_engine()
    cf = np.ascontiguousarray(coeffs, dtype=np.uint64)
    if cf.size % (4 * setup.n):
        raise ValueError("%d coefficients: no whole number of polynomials of %d" % (cf.size // 4, setup.n))
    n = cf.size // (4 * setup.n)
    proof, inf = e.kzg_fk20(setup.points, setup.inf, cf.reshape(-1, 4), setup.log2_n, bitrev)
    return proof.reshape(n, setup.n, 12), inf.reshape(n, setup.n)


class CellSetup:
    """What kzg_cell_proofs_batch needs of a setup for cells of l = 2^log2_l values: the 2N points (l vectors of 2 N / l, and their infinity
    flags) that zkp_kzg_cells_setup derives from the monomial setup [tau^k] g1, k < N.  Build it once per setup and cell size with
    kzg_cells_setup."""

    def __init__(self, points, inf, log2_n, log2_l):
        self.points, self.inf, self.log2_n, self.log2_l = points, inf, int(log2_n), int(log2_l)

    @property
    def n(self):
        return 1 << self.log2_n

    @property
    def l(self):
        return 1 << self.log2_l


def kzg_cells_setup(monomial_g1, log2_l, engine=None):
    """CellSetup of the monomial setup monomial_g1 (N, 12), N a power of two, for cells of 2^log2_l values (zkp_kzg_cells_setup).  The
    points are trusted: check a ceremony's output once with g1_is_valid."""
    e = engine or default_engine()
    mono, log2_n = _pow2_points(monomial_g1, "kzg_cells_setup")
    pts, inf = e.kzg_cells_setup(mono, log2_n, log2_l)
    return CellSetup(pts, inf, log2_n, log2_l)


def _cell_coeffs(setup, coeffs):
    cf = np.ascontiguousarray(coeffs, dtype=np.uint64)
    if cf.size % (4 * setup.n):
        raise ValueError("%d coefficients: no whole number of polynomials of %d" % (cf.size // 4, setup.n))
    return cf.reshape(-1, setup.n, 4)


def kzg_cell_proofs_batch(setup, coeffs, log2_ext=1, bitrev=True, engine=None):
    """(proofs (n, M, 12), inf (n, M)): polynomial j, given by its N coefficients coeffs[j], opened on every coset of l points of its
    domain of D = 2^log2_ext N points by the Feist-Khovratovich multi-proof method (zkp_kzg_cells_batch), M = D / l: proofs[j][m] =
    [q(tau)] g1 with q = (f_j - I) / (X^l - c_m^l), c_m = w_D^m' and m' = bitrev_M(m) with bitrev, as blobs are stored.  setup: a
    CellSetup."""
    e = engine or default_engine()
    cf = _cell_coeffs(setup, coeffs)
    proof, inf = e.kzg_cells(setup.points, setup.inf, cf.reshape(-1, 4), setup.log2_n, setup.log2_l, log2_ext, bitrev)
    return proof.reshape(cf.shape[0], -1, 12), inf.reshape(cf.shape[0], -1)


def kzg_cells_and_proofs_batch(setup, coeffs, log2_ext=1, bitrev=True, engine=None):
    """(cells (n, M, l, 4), proofs (n, M, 12), inf (n, M)): kzg_cell_proofs_batch together with the cells themselves - fr_ntt of the
    coefficients zero-padded to D = 2^log2_ext N, cut into rows of l.  With bitrev (the order blobs are stored in) cell m holds the
    values on the coset of proof m; without it the transform's natural order interleaves the cosets, and the rows are gathered."""
    e = engine or default_engine()
    cf = _cell_coeffs(setup, coeffs)
    n, big_n, l = cf.shape[0], setup.n, setup.l
    big_d = big_n << log2_ext
    big_m = big_d // l
    padded = np.zeros((n, big_d, 4), dtype=np.uint64)
    padded[:, :big_n] = cf
    ev = e.fr_ntt(padded, setup.log2_n + log2_ext, bitrev=bitrev).reshape(n, big_d, 4) if n else padded
    if bitrev:
        cells = ev.reshape(n, big_m, l, 4)
    else:           # value u of cell m is f(w_D^(m + M u))
        cells = np.ascontiguousarray(ev.reshape(n, l, big_m, 4).transpose(0, 2, 1, 3))
    proof, inf = kzg_cell_proofs_batch(setup, cf, log2_ext, bitrev, e)
    return cells, proof, inf


def recover_polynomials_batch(cell_indices, cells, log2_n, log2_l, bitrev=True, engine=None):
    """(coeffs (n, N, 4), ok (n,) int32): blob j back from the cells a client holds of it (zkp_das_recover_batch) - cell_indices[j] the
    distinct indices m < M = 2 N / l it received, cells[j] their values, (len(cell_indices[j]), l, 4), in the same order; N = 2^log2_n,
    l = 2^log2_l, the order of the cells and of the values inside a cell by bitrev as kzg_cells_and_proofs_batch leaves them.  The cells
    are scattered into the dense n x M x l layout and the mask is built from the indices.  ok[j] = 1 iff blob j had at least M / 2 cells
    and they are consistent with a polynomial of degree below N; with too few cells the row is zero, with inconsistent ones unspecified."""
    e = engine or default_engine()
    log2_n, log2_l = int(log2_n), int(log2_l)
    if not 0 <= log2_l <= log2_n:
        raise ValueError("recover_polynomials_batch: 0 <= log2_l <= log2_n expected")
    n, big_n, l = len(cell_indices), 1 << log2_n, 1 << log2_l
    big_m = 2 * big_n // l
    if len(cells) != n:
        raise ValueError("%d index lists for %d lists of cells" % (n, len(cells)))
    values, present = np.zeros((n, big_m, l, 4), dtype=np.uint64), np.zeros((n, big_m), dtype=np.uint8)
    for j in range(n):
        idx = np.ascontiguousarray(cell_indices[j], dtype=np.int64).reshape(-1)
        v = np.ascontiguousarray(cells[j], dtype=np.uint64).reshape(-1, l, 4)
        if v.shape[0] != idx.size:
            raise ValueError("blob %d: %d indices for %d cells" % (j, idx.size, v.shape[0]))
        if idx.size and (idx.min() < 0 or idx.max() >= big_m or np.unique(idx).size != idx.size):
            raise ValueError("blob %d: cell indices must be distinct and below %d" % (j, big_m))
        values[j, idx], present[j, idx] = v, 1
    coeffs, ok = e.das_recover(values.reshape(-1, 4), present.reshape(-1), log2_n, log2_l, bitrev)
    return coeffs.reshape(n, big_n, 4), ok


def recover_cells_and_kzg_proofs_batch(setup, cell_indices, cells, bitrev=True, engine=None):
    """(cells (n, M, l, 4), proofs (n, M, 12), inf (n, M), ok (n,)): every cell and every cell proof of n blobs from any half of their
    cells - recover_polynomials_batch, then kzg_cells_and_proofs_batch on the recovered coefficients (extension 2).  setup: a CellSetup.
    A blob that cannot be recovered is REPORTED, not raised: ok[j] = 0, and its cells and proofs are those of the row the recovery left
    (all zero, hence identity proofs, when fewer than M / 2 cells came; meaningless when the cells were inconsistent) - check ok first."""
    e = engine or default_engine()
    coeffs, ok = recover_polynomials_batch(cell_indices, cells, setup.log2_n, setup.log2_l, bitrev, e)
    out_cells, proof, inf = kzg_cells_and_proofs_batch(setup, coeffs, 1, bitrev, e)
    return out_cells, proof, inf, ok


def _cell_arrays(commitments, cell_index, values, proofs, log2_l):
    c, p = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 12) for x in (commitments, proofs))
    idx = np.ascontiguousarray(cell_index, dtype=np.uint32).reshape(-1)
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 1 << log2_l, 4)
    if not (c.shape[0] == p.shape[0] == idx.shape[0] == v.shape[0]):
        raise ValueError("commitments, cell indices, cells and proofs differ in number")
    return c, idx, v, p


def kzg_cell_verify_batch(monomial_g1_l, g2, tau_l_g2, commitments, cell_index, values, proofs, log2_d, bitrev=True, engine=None, rand=None, inf_c=None,
                          inf_proof=None, points_checked=False, vk_checked=False):
    """True iff every one of the n cells (C_j, m_j, values_j, pi_j) holds against the setup (zkp_kzg_cell_verify_batch: one random
    combination, one MSM call, one final exponentiation; a batch with a false cell passes with probability <= 2^-128).  monomial_g1_l
    (l, 12) = [tau^i] g1, tau_l_g2 = [tau^l] g2; commitments / proofs (n, 12), cell_index (n,), values (n, l, 4), each below r; the
    domain has 2^log2_d points.  kzg_cell_verify_each finds the bad cell when this returns False."""
    e = engine or default_engine()
    mono, log2_l = _pow2_points(monomial_g1_l, "kzg_cell_verify_batch")
    c, idx, v, p = _cell_arrays(commitments, cell_index, values, proofs, log2_l)
    return e.kzg_cell_verify(mono, g2, tau_l_g2, c, idx, v.reshape(-1, 4), p, log2_d, log2_l, bitrev=bitrev, inf_c=inf_c, inf_proof=inf_proof, rand=rand,
                             points_checked=points_checked, vk_checked=vk_checked)


def kzg_cell_verify_each(monomial_g1_l, g2, tau_l_g2, commitments, cell_index, values, proofs, log2_d, bitrev=True, engine=None, inf_c=None, inf_proof=None):
    """bool array (n,): cell j holds.  The per-cell path, composed only of calls that do not know cells: the interpolant's coefficients
    on Python integers (Lagrange's formula on the coset - no transform), -[I_j(tau)] g1 + [c_j^l] pi_j through msm (n sums of l + 1
    terms), C_j added by g1_add, then pairing_check with k = 2 on (C_j - [I_j(tau)] g1 + [c_j^l] pi_j, -g2), (pi_j, [tau^l] g2), ANDed
    with is_valid of every point, with values < r and with cell_index < M."""
    e = engine or default_engine()
    mono, log2_l = _pow2_points(monomial_g1_l, "kzg_cell_verify_each")
    c, idx, v, p = _cell_arrays(commitments, cell_index, values, proofs, log2_l)
    n, l, r = c.shape[0], 1 << log2_l, synthetic.R_ORDER
    log2_m = int(log2_d) - log2_l
    ok = np.ones(n, dtype=bool)
    if n == 0:
        return ok
    g2, tau_l_g2 = (np.ascontiguousarray(x, dtype=np.uint64).reshape(24) for x in (g2, tau_l_g2))
    ic = np.zeros(n, dtype=np.uint8) if inf_c is None else np.ascontiguousarray(inf_c, dtype=np.uint8).reshape(n)
    ip = np.zeros(n, dtype=np.uint8) if inf_proof is None else np.ascontiguousarray(inf_proof, dtype=np.uint8).reshape(n)
    ok &= not (e.g1_is_valid(mono).any() or e.g2_is_valid(np.stack([g2, tau_l_g2])).any())
    ok &= (e.g1_is_valid(c, ic) == 0) & (e.g1_is_valid(p, ip) == 0)
    ok &= synthetic.below_r(v.reshape(-1, 4)).reshape(n, l).all(axis=1) & (idx < (1 << log2_m))
    w_d, w_l = synthetic.fr_root_of_unity(int(log2_d)), synthetic.fr_root_of_unity(log2_l)
    sc = np.zeros((n, l + 1, 4), dtype=np.uint64)
    for j in range(n):
        m = int(idx[j]) & ((1 << log2_m) - 1)
        shift = pow(w_d, synthetic.bit_reverse(m, log2_m) if bitrev else m, r)
        pts = [shift * pow(w_l, synthetic.bit_reverse(u, log2_l) if bitrev else u, r) % r for u in range(l)]
        coef = [0] * l                   # sum_u v_u prod_{t != u} (X - x_t) / (x_u - x_t)
        for u, val in enumerate(synthetic._ints(v[j])):
            num, den = [1], 1
            for t, x in enumerate(pts):
                if t != u:
                    num = [(a - x * b) % r for a, b in zip([0] + num, num + [0])]
                    den = den * (pts[u] - x) % r
            scale = val % r * pow(den, -1, r) % r
            coef = [(a + scale * b) % r for a, b in zip(coef, num)]
        sc[j, :l] = synthetic._rows([-a % r for a in coef])
        sc[j, l] = synthetic._rows([pow(shift, l, r)])[0]
    pts = np.empty((n, l + 1, 12), dtype=np.uint64)
    pts[:, :l], pts[:, l] = mono, p
    inf = np.zeros((n, l + 1), dtype=np.uint8)
    inf[:, l] = ip
    s, s_inf = e.g1_msm(pts.reshape(-1, 12), sc.reshape(-1, 4), n, inf.reshape(-1))
    lhs, lhs_inf = e.g1_add(c, s, ic, s_inf)
    g1 = np.empty((n, 2, 12), dtype=np.uint64)
    q2 = np.empty((n, 2, 24), dtype=np.uint64)
    g1[:, 0], g1[:, 1] = lhs, p
    q2[:, 0], q2[:, 1] = _g2_neg_array(g2), tau_l_g2
    i1 = np.zeros((n, 2), dtype=np.uint8)
    i1[:, 0], i1[:, 1] = lhs_inf, ip
    per, _ = e.pairing_check(g1.reshape(-1, 12), q2.reshape(-1, 24), 2, i1.reshape(-1), np.zeros(2 * n, dtype=np.uint8))
    return ok & (np.asarray(per).reshape(-1) != 0)


def kzg_lagrange_setup(monomial_g1, bitrev=False, engine=None):
    """The Lagrange setup [l_i(tau)] g1 (N, 12) of the N-th roots of unity from the monomial setup [tau^k] g1: the inverse G1 NTT
    (zkp_g1_ntt_batch); with bitrev slot i holds the point of w^bitrev(i), the order blobs use.  Its output goes straight into kzg_commit_batch / kzg_open_batch.  Raises if a point
    comes out infinite, which no honest setup gives."""
    e = engine or default_engine()
    mono, log2_n = _pow2_points(monomial_g1, "kzg_lagrange_setup")
    out, inf = e.g1_ntt(mono, log2_n, inverse=True)
    if np.asarray(inf).any():
        raise ValueError("kzg_lagrange_setup: an infinite Lagrange point (tau is a root of unity, or the setup is malformed)")
    if bitrev:      # ZKP_NTT_BITREV orders the INPUT of an inverse transform; here the output side is the evaluation side: N rows, once per setup
        out = out[[int(format(i, "0%db" % log2_n)[::-1], 2) if log2_n else 0 for i in range(1 << log2_n)]]
    return np.ascontiguousarray(out)


def kzg_verify_blob_batch(setup, evals, commitments, z, proofs, bitrev=True, engine=None, rand=None):
    """True iff proof j opens commitment j at z_j to the value of polynomial j there, the polynomial given by its N = 2^k evaluations
    evals[j] over the N-th roots of unity (bit-reversed order with bitrev, the order blobs are stored in): y = fr_eval(evals, z) on
    the device, then kzg_verify_batch on the same tensors - nothing returns to the host in between.  evals (n, N, 4)."""
    import torch
    e = engine or default_engine()
    ev = np.ascontiguousarray(evals, dtype=np.uint64)
    n = np.ascontiguousarray(z, dtype=np.uint64).size // 4
    if n == 0:
        return True
    big_n = ev.size // 4 // n
    log2_n = big_n.bit_length() - 1
    if big_n < 1 or big_n != 1 << log2_n or ev.size != n * big_n * 4:
        raise ValueError("evals hold %d elements for %d polynomials" % (ev.size // 4, n))
    dev = torch.device("cuda", e.device)
    t = lambda a, w: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, w).view(np.int64)).to(dev)
    tz = t(z, 4)
    ty = e.fr_eval(t(ev, 4), tz, log2_n, bitrev)
    flag = e.kzg_verify_batch(*[t(a, w) for a, w in zip(setup.arrays(), (12, 24, 24))], t(commitments, 12), tz, ty, t(proofs, 12), rand=rand)
    return bool(flag.item())


# ------------------------------------------------------------------------------------------------ BLS signatures (include/zkp_bls.h)
ETH_DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"


def hash_to_g2(msgs, dst, engine=None):
    """a list of messages (bytes) -> (points (n, 24), inf (n,)): RFC 9380 BLS12381G2_XMD:SHA-256_SSWU_RO_ under the tag dst"""
    return (engine or default_engine()).hash_to_g2(msgs, dst)


def bls_sign_batch(sks, msgs, dst, engine=None):
    """sig_i = [sk_i] H(m_i): secret keys (n, 4) words below r, messages a list of bytes -> (signatures (n, 24), inf (n,))"""
    e = engine or default_engine()
    h, hinf = e.hash_to_g2(msgs, dst)
    sks = np.ascontiguousarray(sks, dtype=np.uint64).reshape(-1, 4)
    if sks.shape[0] != h.shape[0]:
        raise ValueError("%d secret keys for %d messages" % (sks.shape[0], h.shape[0]))
    if h.shape[0] == 0:
        return h, hinf
    sig, inf = e.g2_mul(h, sks)
    inf = inf | hinf
    sig[inf != 0] = 0
    sig[inf != 0, 12] = 1
    return sig, inf


def bls_verify_batch(pks, msgs, sigs, dst, rand=None, points_checked=False, inf_pk=None, inf_sig=None, engine=None):
    """True iff every signature verifies (one pairing product under a random linear combination, PairingEngine.bls_verify): public keys
    (n, 12) in G1, messages a list of bytes, signatures (n, 24) in G2"""
    return (engine or default_engine()).bls_verify(pks, msgs, sigs, dst, inf_pk=inf_pk, inf_sig=inf_sig, rand=rand, points_checked=points_checked)


def bls_verify_each(pks, msgs, sigs, dst, points_checked=False, inf_pk=None, inf_sig=None, engine=None):
    """bool array (n,): signature i verifies.  The per-signature path, the way groth16_verify_each locates failures: pairing_check with
    k = 2 on (pk_i, H(m_i)), (-g1, sig_i), ANDed with is_valid of pk_i and sig_i (unless points_checked) and with pk_i not the identity."""
    e = engine or default_engine()
    pks = np.ascontiguousarray(pks, dtype=np.uint64).reshape(-1, 12)
    sigs = np.ascontiguousarray(sigs, dtype=np.uint64).reshape(-1, 24)
    n = pks.shape[0]
    if sigs.shape[0] != n or len(msgs) != n:
        raise ValueError("%d messages, %d public keys, %d signatures" % (len(msgs), n, sigs.shape[0]))
    ok = np.ones(n, dtype=bool)
    if n == 0:
        return ok
    ip = np.zeros(n, dtype=np.uint8) if inf_pk is None else np.ascontiguousarray(inf_pk, dtype=np.uint8).reshape(n)
    isg = np.zeros(n, dtype=np.uint8) if inf_sig is None else np.ascontiguousarray(inf_sig, dtype=np.uint8).reshape(n)
    ok &= ip == 0
    if not points_checked:
        ok &= (e.g1_is_valid(pks, ip) == 0) & (e.g2_is_valid(sigs, isg) == 0)
    h, hinf = e.hash_to_g2(msgs, dst)
    g1 = np.empty((n, 2, 12), dtype=np.uint64)
    g2 = np.empty((n, 2, 24), dtype=np.uint64)
    g1[:, 0], g1[:, 1] = pks, (-G1Affine.generator()).to_array()
    g2[:, 0], g2[:, 1] = h, sigs
    i1, i2 = np.zeros((n, 2), dtype=np.uint8), np.zeros((n, 2), dtype=np.uint8)
    i1[:, 0], i2[:, 0], i2[:, 1] = ip, hinf, isg
    per, _ = e.pairing_check(g1.reshape(-1, 12), g2.reshape(-1, 24), 2, i1.reshape(-1), i2.reshape(-1))
    return ok & (np.asarray(per).reshape(-1) != 0)


def _bls_decompress(pk_bytes, sig_bytes, e):
    pk, ipk, spk = e.decompress_points(pk_bytes, 1)
    sg, isg, ssg = e.decompress_points(sig_bytes, 2)
    return pk, ipk, sg, isg, (np.asarray(spk) == 0) & (np.asarray(ssg) == 0)


def bls_verify_batch_compressed(pk_bytes, msgs, sig_bytes, dst, rand=None, engine=None):
    """bls_verify_batch on 48-byte compressed public keys and 96-byte compressed signatures, decompressed on the GPU; a string that does
    not decompress fails the batch"""
    e = engine or default_engine()
    pk, ipk, sg, isg, dec = _bls_decompress(pk_bytes, sig_bytes, e)
    if not dec.all():
        return False
    return e.bls_verify(pk, msgs, sg, dst, inf_pk=ipk, inf_sig=isg, rand=rand)


def bls_verify_each_compressed(pk_bytes, msgs, sig_bytes, dst, engine=None):
    e = engine or default_engine()
    pk, ipk, sg, isg, dec = _bls_decompress(pk_bytes, sig_bytes, e)
    return dec & bls_verify_each(pk, msgs, sg, dst, inf_pk=ipk, inf_sig=isg, engine=e)


# ------------------------------------------------------------------------------------------------ min-sig BLS signatures (include/zkp_bls_minsig.h)
QUICKNET_DST = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"


def hash_to_g1(msgs, dst, engine=None):
    """a list of messages (bytes) -> (points (n, 12), inf (n,)): RFC 9380 BLS12381G1_XMD:SHA-256_SSWU_RO_ under the tag dst"""
    return (engine or default_engine()).hash_to_g1(msgs, dst)


def bls_minsig_keygen_batch(sks, engine=None):
    """pk_i = [sk_i] g2: secret keys (n, 4) words below r -> (public keys (n, 24), inf (n,))"""
    e = engine or default_engine()
    sks = np.ascontiguousarray(sks, dtype=np.uint64).reshape(-1, 4)
    return e.g2_mul(G2Affine.generator().to_array(), sks)


def bls_minsig_sign_batch(sks, msgs, dst, engine=None):
    """sig_i = [sk_i] H(m_i) in G1: secret keys (n, 4) words below r, messages a list of bytes -> (signatures (n, 12), inf (n,))"""
    e = engine or default_engine()
    h, hinf = e.hash_to_g1(msgs, dst)
    sks = np.ascontiguousarray(sks, dtype=np.uint64).reshape(-1, 4)
    if sks.shape[0] != h.shape[0]:
        raise ValueError("%d secret keys for %d messages" % (sks.shape[0], h.shape[0]))
    if h.shape[0] == 0:
        return h, hinf
    sig, inf = e.g1_mul(h, sks)
    inf = inf | hinf
    sig[inf != 0] = 0
    sig[inf != 0, 6] = 1
    return sig, inf


def bls_minsig_verify_batch(pks, msgs, sigs, dst, rand=None, points_checked=False, inf_pk=None, inf_sig=None, engine=None):
    """True iff every signature verifies (one pairing product under a random linear combination, PairingEngine.bls_minsig_verify):
    public keys (n, 24) in G2, messages a list of bytes, signatures (n, 12) in G1"""
    return (engine or default_engine()).bls_minsig_verify(pks, msgs, sigs, dst, inf_pk=inf_pk, inf_sig=inf_sig, rand=rand, points_checked=points_checked)


def bls_minsig_verify_samekey_batch(pk, msgs, sigs, dst, rand=None, points_checked=False, inf_sig=None, engine=None):
    """bls_minsig_verify_batch when ONE public key pk (24 words) signed every message - a beacon chain: two G1 sums and two Miller loops
    for the whole batch (PairingEngine.bls_minsig_verify_samekey)"""
    return (engine or default_engine()).bls_minsig_verify_samekey(pk, msgs, sigs, dst, inf_sig=inf_sig, rand=rand, points_checked=points_checked)


def bls_minsig_verify_each(pks, msgs, sigs, dst, points_checked=False, inf_pk=None, inf_sig=None, engine=None):
    """bool array (n,): signature i verifies.  The per-signature path of bls_verify_each: pairing_check with k = 2 on (H(m_i), pk_i),
    (sig_i, -g2), ANDed with is_valid of pk_i and sig_i (unless points_checked) and with pk_i not the identity."""
    e = engine or default_engine()
    pks = np.ascontiguousarray(pks, dtype=np.uint64).reshape(-1, 24)
    sigs = np.ascontiguousarray(sigs, dtype=np.uint64).reshape(-1, 12)
    n = pks.shape[0]
    if sigs.shape[0] != n or len(msgs) != n:
        raise ValueError("%d messages, %d public keys, %d signatures" % (len(msgs), n, sigs.shape[0]))
    ok = np.ones(n, dtype=bool)
    if n == 0:
        return ok
    ip = np.zeros(n, dtype=np.uint8) if inf_pk is None else np.ascontiguousarray(inf_pk, dtype=np.uint8).reshape(n)
    isg = np.zeros(n, dtype=np.uint8) if inf_sig is None else np.ascontiguousarray(inf_sig, dtype=np.uint8).reshape(n)
    ok &= ip == 0
    if not points_checked:
        ok &= (e.g2_is_valid(pks, ip) == 0) & (e.g1_is_valid(sigs, isg) == 0)
    h, hinf = e.hash_to_g1(msgs, dst)
    g1 = np.empty((n, 2, 12), dtype=np.uint64)
    g2 = np.empty((n, 2, 24), dtype=np.uint64)
    g1[:, 0], g1[:, 1] = h, sigs
    g2[:, 0], g2[:, 1] = pks, (-G2Affine.generator()).to_array()
    i1, i2 = np.zeros((n, 2), dtype=np.uint8), np.zeros((n, 2), dtype=np.uint8)
    i1[:, 0], i1[:, 1], i2[:, 0] = hinf, isg, ip
    per, _ = e.pairing_check(g1.reshape(-1, 12), g2.reshape(-1, 24), 2, i1.reshape(-1), i2.reshape(-1))
    return ok & (np.asarray(per).reshape(-1) != 0)


def _bls_minsig_decompress(pk_bytes, sig_bytes, e):
    pk, ipk, spk = e.decompress_points(pk_bytes, 2)
    sg, isg, ssg = e.decompress_points(sig_bytes, 1)
    return pk, ipk, sg, isg, (np.asarray(spk) == 0) & (np.asarray(ssg) == 0)


def bls_minsig_verify_batch_compressed(pk_bytes, msgs, sig_bytes, dst, rand=None, engine=None):
    """bls_minsig_verify_batch on 96-byte compressed public keys and 48-byte compressed signatures, decompressed on the GPU; a string
    that does not decompress fails the batch"""
    e = engine or default_engine()
    pk, ipk, sg, isg, dec = _bls_minsig_decompress(pk_bytes, sig_bytes, e)
    if not dec.all():
        return False
    return e.bls_minsig_verify(pk, msgs, sg, dst, inf_pk=ipk, inf_sig=isg, rand=rand)


def bls_minsig_verify_each_compressed(pk_bytes, msgs, sig_bytes, dst, engine=None):
    e = engine or default_engine()
    pk, ipk, sg, isg, dec = _bls_minsig_decompress(pk_bytes, sig_bytes, e)
    return dec & bls_minsig_verify_each(pk, msgs, sg, dst, inf_pk=ipk, inf_sig=isg, engine=e)


# ------------------------------------------------------------------------------------------------ committee aggregation (include/zkp_bls_agg.h)
SUBTRACT = 0x80000000   # bit 31 of an entry: subtract the table row


def committee_entries(committees, bits=None, absent_from=None):
    """Lists of table rows, one list per committee -> (idx uint32, seg_off uint64 (n + 1,)): the entries of g1_segment_sum and
    bls_fast_aggregate_verify.  bits: one aggregation bitfield per committee (a sequence of 0 / 1, one per member): only the members whose
    bit is set enter.  absent_from: the table row that holds the total of a committee (one row, or one per committee): the lists then name
    the ABSENT members, and committee i becomes (+total_i, -a, -b, ...), "the aggregate of all minus the absent"."""
    if bits is not None and absent_from is not None:
        raise ValueError("bits selects the members that signed, absent_from takes the lists as the members that did not: give one")
    committees = [list(c) for c in committees]
    if bits is not None:
        if len(bits) != len(committees) or any(len(b) != len(c) for b, c in zip(bits, committees)):
            raise ValueError("one bit per member of every committee")
        committees = [[r for r, b in zip(c, bs) if b] for c, bs in zip(committees, bits)]
    for c in committees:
        if any(not 0 <= int(r) < SUBTRACT for r in c):
            raise ValueError("table rows lie in [0, 2^31)")
    if absent_from is not None:
        totals = [absent_from] * len(committees) if np.isscalar(absent_from) else list(absent_from)
        if len(totals) != len(committees) or any(not 0 <= int(t) < SUBTRACT for t in totals):
            raise ValueError("one total row in [0, 2^31) per committee")
        committees = [[int(t)] + [int(r) | SUBTRACT for r in c] for t, c in zip(totals, committees)]
    seg_off = np.zeros(len(committees) + 1, dtype=np.uint64)
    if committees:
        seg_off[1:] = np.cumsum([len(c) for c in committees], dtype=np.uint64)
    idx = np.array([int(r) for c in committees for r in c], dtype=np.uint32)
    return idx, seg_off


def _entries(committees, bits, absent_from):
    """committees as lists of rows (through committee_entries), or the ready pair (idx, seg_off) of arrays"""
    if isinstance(committees, tuple) and len(committees) == 2 and isinstance(committees[0], np.ndarray):
        if bits is not None or absent_from is not None:
            raise ValueError("bits and absent_from shape lists of rows, not ready entries")
        return (np.ascontiguousarray(committees[0], dtype=np.uint32).reshape(-1), np.ascontiguousarray(committees[1], dtype=np.uint64).reshape(-1))
    return committee_entries(committees, bits, absent_from)


def bls_aggregate_keys(table, committees, bits=None, absent_from=None, engine=None):
    """the committees' aggregate public keys: (points (n, 12), inf (n,)) (PairingEngine.g1_segment_sum on committee_entries; committees
    may also be a ready (idx, seg_off) pair)"""
    idx, seg_off = _entries(committees, bits, absent_from)
    out, inf, _ = (engine or default_engine()).g1_segment_sum(table, idx, seg_off)
    return out, inf


def bls_fast_aggregate_verify_batch(table, committees, msgs, sigs, dst, bits=None, absent_from=None, rand=None, points_checked=False, inf_sig=None,
                                    engine=None):
    """True iff every aggregate signature verifies under the sum of its committee's keys (PairingEngine.bls_fast_aggregate_verify): table
    (n_table, 12) validated public keys, committees lists of rows (committee_entries) or a ready (idx, seg_off) pair, messages a list of
    bytes, signatures (n, 24)"""
    idx, seg_off = _entries(committees, bits, absent_from)
    return (engine or default_engine()).bls_fast_aggregate_verify(table, idx, seg_off, msgs, sigs, dst, inf_sig=inf_sig, rand=rand,
                                                                  points_checked=points_checked)


def bls_fast_aggregate_verify_each(table, committees, msgs, sigs, dst, bits=None, absent_from=None, points_checked=False, inf_sig=None, engine=None):
    """bool array (n,): aggregate i verifies - the segment sums, then bls_verify_each on them, ANDed with the statuses and with the
    committee not being empty"""
    e = engine or default_engine()
    idx, seg_off = _entries(committees, bits, absent_from)
    apk, inf, st = e.g1_segment_sum(table, idx, seg_off)
    ok = bls_verify_each(apk, msgs, sigs, dst, points_checked=points_checked, inf_pk=inf, inf_sig=inf_sig, engine=e)
    return ok & (np.asarray(st) == 0) & (np.diff(seg_off.astype(np.int64)) > 0)


# ------------------------------------------------------------------------------------------------ G2 aggregation and AggregateVerify (include/zkp_bls_agg_g2.h)
def bls_aggregate_signatures(sigs, groups, bits=None, absent_from=None, engine=None):
    """Aggregate: the sums of min-pk signatures, (points (n, 24), inf (n,)) (PairingEngine.g2_segment_sum).  sigs (n_sig, 24) finite points
    of G2, groups lists of rows of sigs (through committee_entries, with its bits and absent_from) or a ready (idx, seg_off) pair"""
    idx, seg_off = _entries(groups, bits, absent_from)
    out, inf, _ = (engine or default_engine()).g2_segment_sum(sigs, idx, seg_off)
    return out, inf


def bls_minsig_aggregate_keys(table, committees, bits=None, absent_from=None, engine=None):
    """bls_aggregate_keys for the minimal-signature-size layout: the committees' aggregate public keys in G2, (points (n, 24), inf (n,))"""
    idx, seg_off = _entries(committees, bits, absent_from)
    out, inf, _ = (engine or default_engine()).g2_segment_sum(table, idx, seg_off)
    return out, inf


def bls_minsig_fast_aggregate_verify_batch(table, committees, msgs, sigs, dst, bits=None, absent_from=None, rand=None, points_checked=False, inf_sig=None,
                                           engine=None):
    """bls_fast_aggregate_verify_batch for the minimal-signature-size layout (PairingEngine.bls_minsig_fast_aggregate_verify): table
    (n_table, 24) validated public keys in G2, signatures (n, 12) in G1"""
    idx, seg_off = _entries(committees, bits, absent_from)
    return (engine or default_engine()).bls_minsig_fast_aggregate_verify(table, idx, seg_off, msgs, sigs, dst, inf_sig=inf_sig, rand=rand,
                                                                         points_checked=points_checked)


def bls_minsig_fast_aggregate_verify_each(table, committees, msgs, sigs, dst, bits=None, absent_from=None, points_checked=False, inf_sig=None, engine=None):
    """bool array (n,): aggregate i verifies - the G2 segment sums, then bls_minsig_verify_each on them, ANDed with the statuses and with
    the committee not being empty"""
    e = engine or default_engine()
    idx, seg_off = _entries(committees, bits, absent_from)
    apk, inf, st = e.g2_segment_sum(table, idx, seg_off)
    ok = bls_minsig_verify_each(apk, msgs, sigs, dst, points_checked=points_checked, inf_pk=inf, inf_sig=inf_sig, engine=e)
    return ok & (np.asarray(st) == 0) & (np.diff(seg_off.astype(np.int64)) > 0)


def bls_aggregate_verify_batch(pks, msgs, seg_off, sigs, dst, rand=None, points_checked=False, inf_pk=None, inf_sig=None, engine=None):
    """AggregateVerify, batched: True iff every signature j (sigs (n, 24)) verifies over the pairs (pks[i], msgs[i]) for i in
    [seg_off[j], seg_off[j + 1]) (PairingEngine.bls_aggregate_verify): public keys (n_msg, 12), messages a list of n_msg bytes, seg_off
    (n + 1,).  A segment without a pair fails the batch.  The messages of one signature are not tested for distinctness (the
    proof-of-possession scheme); the basic scheme's rule is the caller's."""
    return (engine or default_engine()).bls_aggregate_verify(pks, msgs, seg_off, sigs, dst, inf_pk=inf_pk, inf_sig=inf_sig, rand=rand,
                                                             points_checked=points_checked)


def bls_aggregate_verify_each(pks, msgs, seg_off, sigs, dst, points_checked=False, inf_pk=None, inf_sig=None, engine=None):
    """bool array (n,): signature j verifies over its pairs.  One bls_verify call per segment on an expansion built here: the signature
    under the segment's first message, the flagged identity under the others, rand rows (1, 0).  An empty segment is False."""
    e = engine or default_engine()
    pks = np.ascontiguousarray(pks, dtype=np.uint64).reshape(-1, 12)
    sigs = np.ascontiguousarray(sigs, dtype=np.uint64).reshape(-1, 24)
    off = np.ascontiguousarray(seg_off, dtype=np.uint64).reshape(-1)
    n, n_msg = sigs.shape[0], pks.shape[0]
    if off.size != n + 1 or len(msgs) != n_msg:
        raise ValueError("%d messages, %d public keys; %d offsets for %d signatures" % (len(msgs), n_msg, off.size, n))
    if int(off[0]) != 0 or int(off[-1]) != n_msg or (n and bool((off[1:] < off[:-1]).any())):
        raise ValueError("seg_off does not run from 0 to the number of messages without decreasing")
    ip = np.zeros(n_msg, dtype=np.uint8) if inf_pk is None else np.ascontiguousarray(inf_pk, dtype=np.uint8).reshape(n_msg)
    isg = np.zeros(n, dtype=np.uint8) if inf_sig is None else np.ascontiguousarray(inf_sig, dtype=np.uint8).reshape(n)
    ok = np.zeros(n, dtype=bool)
    for j in range(n):
        lo, hi = int(off[j]), int(off[j + 1])
        k = hi - lo
        if k == 0:
            continue
        xs = np.zeros((k, 24), dtype=np.uint64)
        xs[:, 12] = 1
        xs[0] = sigs[j]
        xi = np.ones(k, dtype=np.uint8)
        xi[0] = isg[j]
        r = np.zeros((k, 2), dtype=np.uint64)
        r[:, 0] = 1
        ok[j] = e.bls_verify(pks[lo:hi], list(msgs[lo:hi]), xs, dst, inf_pk=ip[lo:hi], inf_sig=xi, rand=r, points_checked=points_checked)
    return ok


# ------------------------------------------------------------------------------------------------ verification grouped by message (include/zkp_bls_grouped.h)
def group_by_message(messages):
    """A list of n messages (bytes) -> (perm int64 (n,), distinct (list of m bytes), grp_off uint64 (m + 1,)): the order bls_verify_grouped
    wants.  The distinct messages keep the order of their first appearance and the signatures of one message their order: signatures
    perm[grp_off[g] : grp_off[g + 1]] sign distinct[g]."""
    first, members = {}, []
    for i, msg in enumerate(messages):
        msg = bytes(msg)
        g = first.setdefault(msg, len(members))
        if g == len(members):
            members.append([])
        members[g].append(i)
    distinct = [None] * len(members)
    for msg, g in first.items():
        distinct[g] = msg
    grp_off = np.zeros(len(members) + 1, dtype=np.uint64)
    if members:
        grp_off[1:] = np.cumsum([len(x) for x in members], dtype=np.uint64)
    perm = np.array([i for x in members for i in x], dtype=np.int64)
    return perm, distinct, grp_off


def _take(rows, perm, cols=None, dtype=np.uint64):
    if rows is None:
        return None
    rows = np.ascontiguousarray(rows, dtype=dtype)
    return np.ascontiguousarray((rows.reshape(-1, cols) if cols else rows.reshape(-1))[perm])


def bls_verify_grouped_batch(pks, msgs, sigs, dst, rand=None, points_checked=False, inf_pk=None, inf_sig=None, engine=None):
    """bls_verify_batch with one hash and one Miller pair per DISTINCT message (PairingEngine.bls_verify_grouped): the arguments and the
    answer of bls_verify_batch; the signatures are put in the order of group_by_message here, rand (per signature, in the caller's order)
    with them"""
    perm, distinct, grp_off = group_by_message(msgs)
    pks, sigs = _take(pks, perm, 12), _take(sigs, perm, 24)
    if pks.shape[0] != perm.size or sigs.shape[0] != perm.size:
        raise ValueError("%d messages, %d public keys, %d signatures" % (perm.size, pks.shape[0], sigs.shape[0]))
    return (engine or default_engine()).bls_verify_grouped(pks, grp_off, distinct, sigs, dst, inf_pk=_take(inf_pk, perm, dtype=np.uint8),
                                                           inf_sig=_take(inf_sig, perm, dtype=np.uint8), rand=_take(rand, perm, 2),
                                                           points_checked=points_checked)


def bls_fast_aggregate_verify_grouped_batch(table, committees, msgs, sigs, dst, bits=None, absent_from=None, rand=None, points_checked=False, inf_sig=None,
                                            engine=None):
    """bls_fast_aggregate_verify_batch with one hash and one Miller pair per DISTINCT message (PairingEngine.bls_fast_aggregate_verify_grouped):
    the arguments and the answer of bls_fast_aggregate_verify_batch; committees, signatures and rand are put in the order of
    group_by_message here"""
    idx, seg_off = _entries(committees, bits, absent_from)
    perm, distinct, grp_off = group_by_message(msgs)
    if seg_off.size - 1 != perm.size:
        raise ValueError("%d committees, %d messages" % (seg_off.size - 1, perm.size))
    lo, hi = seg_off[:-1].astype(np.int64)[perm], seg_off[1:].astype(np.int64)[perm]
    new_off = np.zeros(perm.size + 1, dtype=np.uint64)
    if perm.size:
        new_off[1:] = np.cumsum(hi - lo).astype(np.uint64)
    new_idx = np.concatenate([idx[a:b] for a, b in zip(lo, hi)]).astype(np.uint32) if perm.size else idx[:0]
    return (engine or default_engine()).bls_fast_aggregate_verify_grouped(table, new_idx, new_off, grp_off, distinct, _take(sigs, perm, 24), dst,
                                                                          inf_sig=_take(inf_sig, perm, dtype=np.uint8), rand=_take(rand, perm, 2),
                                                                          points_checked=points_checked)
