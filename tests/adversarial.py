"""Adversarial operand pool for the field, tower and inversion kernels (tests/test_adversarial_cpu.py, tests/test_gpu_adversarial.py).
Deterministic, built from p and the limb geometries of the code alone; nothing here imports the library or touches a GPU.

Every value is canonical (0 <= v < p) and carries a class and a name, so that a failing case names where it came from:
  ends       the ends of the canonical range
  limbs      limb boundaries of every geometry in the code: 14 x 28 bits (cooperative core), 12 x 32 (thread core), 13 x 30 (division
             steps), 6 x 64 (wire), all-ones / alternating limb patterns, extreme balanced digits of the 28-bit core
  pow2       2^k, 2^k - 1, p - 2^k for every k < 381
  pre28/32   Montgomery pre-images V R^-1 of the values V of the classes above for R = 2^392 (28-bit core) and R = 2^384 (32-bit
             core): the g the division steps of f_inv start from (the canonical value of a R) is the structured value V.  The
             STORED representative is V or V + p (the load's reduction ends in [0, p + p / 2^11)); preimages28_verified() is the
             subset where the 28-bit core's emulator holds exactly the digits of V.  The pool keeps them all: every one starts
             the inversion from V, and V + p is a structured operand of the lazy core in its own right
  pairs      result-targeted pairs: a + b in {p-1, p, p+1}, a - b in {-1, 0, 1}, a b and a^2 in {0, 1, p-1, 2, (p+1)/2}
  searched   vectors tests/golden/gen_adversarial.py found on the CPU models (tests/golden/adversarial_operands.json)"""
import json
import os
from collections import namedtuple

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
PBITS = 381
GEOMETRIES = {"w28": (28, 14), "w32": (32, 12), "w30": (30, 13), "w64": (64, 6)}      # name -> (limb width, limbs)
R28, R32 = 1 << 392, 1 << 384                                                         # Montgomery radices of the two cores
JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adversarial_operands.json")

Op = namedtuple("Op", "cls name v")


def _dedupe(ops):
    seen, out = set(), []
    for o in ops:
        assert 0 <= o.v < P, o
        if o.v not in seen:
            seen.add(o.v)
            out.append(o)
    return out


def ends():
    vals = (("0", 0), ("1", 1), ("2", 2), ("3", 3), ("p-1", P - 1), ("p-2", P - 2), ("p-3", P - 3), ("(p-1)/2", (P - 1) // 2),
            ("(p+1)/2", (P + 1) // 2))
    return [Op("ends", n, v) for n, v in vals]


def limb_boundaries():
    out = []
    for g, (w, n) in GEOMETRIES.items():
        ones = (1 << w) - 1
        for i in range(1, n):
            if w * i - 1 >= PBITS:
                break
            for nm, v in (("2^(%d*%d)" % (w, i), 1 << (w * i)), ("2^(%d*%d)+1" % (w, i), (1 << (w * i)) + 1),
                          ("2^(%d*%d)-1" % (w, i), (1 << (w * i)) - 1), ("2^(%d*%d-1)" % (w, i), 1 << (w * i - 1)),
                          ("2^(%d*%d-1)+1" % (w, i), (1 << (w * i - 1)) + 1), ("2^(%d*%d-1)-1" % (w, i), (1 << (w * i - 1)) - 1)):
                if v < P:
                    out.append(Op("limbs", "%s:%s" % (g, nm), v))
                    out.append(Op("limbs", "%s:p-(%s)" % (g, nm), P - v))
        # all-ones in every limb below the top: the largest value < p with that pattern
        low = (1 << (w * (n - 1))) - 1
        top = (P >> (w * (n - 1))) - (1 if low >= (P & low) else 0)
        out.append(Op("limbs", "%s:ones-below-top" % g, (top << (w * (n - 1))) | low))
        out.append(Op("limbs", "%s:ones-below-top,top=0" % g, low))
        for par in (0, 1):                 # alternating all-ones / zero limbs, cut to 380 bits so that the value stays below p
            v = sum(ones << (w * i) for i in range(n) if i % 2 == par) & ((1 << (PBITS - 1)) - 1)
            out.append(Op("limbs", "%s:alternating-%s" % (g, "even" if par == 0 else "odd"), v))
    # the balanced core: the 13 digits below the top all +(2^27 - 1) or all -2^27, with the smallest and the largest top digit
    w, n = GEOMETRIES["w28"]
    ptop = P >> (w * (n - 1))
    hi = sum(((1 << 27) - 1) << (w * i) for i in range(n - 1))
    lo = -sum((1 << 27) << (w * i) for i in range(n - 1))
    for nm, base, tops in (("+max", hi, (0, 1, ptop - 1, ptop)), ("-min", lo, (1, 2, ptop, ptop + 1))):
        for t in tops:
            v = base + (t << (w * (n - 1)))
            if 0 <= v < P:
                out.append(Op("limbs", "w28:balanced-digits%s,top=%d" % (nm, t), v))
    return out


def powers_of_two():
    out = []
    for k in range(PBITS):
        out.append(Op("pow2", "2^%d" % k, 1 << k))
        out.append(Op("pow2", "2^%d-1" % k, (1 << k) - 1))
        out.append(Op("pow2", "p-2^%d" % k, P - (1 << k)))
    return out


def preimages(ops, radix, cls):
    """for every structured V: the canonical a with a * radix = V (mod p) - its Montgomery form is V"""
    rinv = pow(radix, -1, P)
    return [Op(cls, "%s/R[%s]" % (o.name, o.cls), o.v * rinv % P) for o in ops]


def balanced28(v):
    """|v| < 2^391 -> its 14 balanced digits (low 13 in [-2^27, 2^27)), as the 28-bit core's reduction leaves them"""
    out = []
    for _ in range(13):
        d = ((v + (1 << 27)) & ((1 << 28) - 1)) - (1 << 27)
        out.append(d)
        v = (v - d) >> 28
    return out + [v]


_VERIFIED28 = None


def preimages28_verified(ops=None):
    """the R = 2^392 pre-images whose LOADED slot on the cooperative core's emulator (wire -> Montgomery, tools/coopgen.py) holds
    exactly the balanced digits of the intended V; the others (the load left V - p or V + p in the slot) are dropped"""
    global _VERIFIED28
    if ops is None and _VERIFIED28 is not None:
        return _VERIFIED28
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import coopgen as cg
    src = structured() if ops is None else ops
    pre = preimages(src, R28, "pre28")
    prog = cg.prog_tower_to_state().steps
    keep = []
    for i in range(0, len(src), 12):
        chunk = pre[i:i + 12]
        wire = [o.v for o in chunk] + [0] * (12 - len(chunk))
        st = cg.Emu(wire_in=wire).run(prog).state
        for j, o in enumerate(chunk):
            if list(st[j]) == balanced28(src[i + j].v):
                keep.append(o)
    if ops is None:
        _VERIFIED28 = keep
    return keep


def structured():
    """classes ends + limbs + pow2, without repeated values"""
    return _dedupe(ends() + limb_boundaries() + powers_of_two())


def cross_set():
    """what the binary field operations take as a full cross product: ends, limbs, their pre-images on both cores"""
    base = _dedupe(ends() + limb_boundaries())
    return _dedupe(base + preimages(base, R28, "pre28") + preimages(base, R32, "pre32"))


def pool():
    """every single-value class: ends, limbs, pow2, pre28, pre32 (searched values are added by the tests that load the JSON)"""
    s = structured()
    return _dedupe(s + preimages(s, R28, "pre28") + preimages(s, R32, "pre32"))


SUM_TARGETS = (("a+b=p-1", P - 1), ("a+b=p", P), ("a+b=p+1", P + 1))
DIFF_TARGETS = (("a-b=-1", -1), ("a-b=0", 0), ("a-b=1", 1))
PROD_TARGETS = (("0", 0), ("1", 1), ("p-1", P - 1), ("2", 2), ("(p+1)/2", (P + 1) // 2))


def targeted_pairs(ops=None):
    """-> {target name: [(name of a, a, b)]}; every pair canonical, every pair hits its target exactly"""
    ops = structured() if ops is None else ops
    out = {}
    for nm, t in SUM_TARGETS:
        out[nm] = [(o.name, o.v, t - o.v) for o in ops if 0 <= t - o.v < P]
    for nm, t in DIFF_TARGETS:
        out[nm] = [(o.name, o.v, o.v - t) for o in ops if 0 <= o.v - t < P]
    for nm, t in PROD_TARGETS:
        out["ab=" + nm] = [(o.name, o.v, t * pow(o.v, -1, P) % P if o.v else 0) for o in ops if o.v or t == 0]
        roots = []
        if pow(t, (P - 1) // 2, P) in (0, 1):                   # p = 3 mod 4: a root is t^((p+1)/4)
            r = pow(t, (P + 1) // 4, P)
            roots = [("sqrt(%s)" % nm, r, r)] + ([("-sqrt(%s)" % nm, P - r, P - r)] if r else [])
        out["a^2=" + nm] = roots
    return out


def core_values():
    """a small subset for the tower records: the ends, the limb patterns, one boundary pair per geometry and their pre-images"""
    lb = limb_boundaries()
    pick = [o for o in lb if "ones" in o.name or "alternating" in o.name or "balanced" in o.name]
    for g, (w, n) in GEOMETRIES.items():
        i = n // 2
        pick += [o for o in lb if o.name in ("%s:2^(%d*%d)-1" % (g, w, i), "%s:p-(2^(%d*%d))" % (g, w, i), "%s:2^(%d*%d-1)" % (g, w, n - 1))]
    base = _dedupe(ends() + pick)
    return _dedupe(base + preimages(base, R28, "pre28") + preimages(base, R32, "pre32"))


class _Rng:
    """SplitMix64: the seeded generator of the record draws (the same stream everywhere, no dependence on Python's random)"""

    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def below(self, n):
        return self.next() % n


def records(width=12, seed=0xAD7E, n_drawn=96):
    """tower records of `width` Fp coefficients (2: Fp2, 6: Fp6, 12: Fp12) as (shape name, [12 ints]); coefficients behind `width`
    are zero, as the header asks.  Shapes: every coefficient the same value; two values alternating by coefficient; one-hot and
    one-cold at each position; each embedded subfield; coefficients drawn from the whole pool by a seeded generator."""
    core = core_values()
    full = pool()
    out = []
    pad = lambda c: list(c) + [0] * (12 - len(c))
    for o in core:
        out.append(("uniform[%s]" % o.name, pad([o.v] * width)))
    for a, b in zip(core, core[1:] + core[:1]):
        out.append(("alternating[%s|%s]" % (a.name, b.name), pad([a.v if i % 2 == 0 else b.v for i in range(width)])))
    few = [o for o in core if o.cls == "ends"][3:8] + [o for o in core if "ones-below-top" in o.name and o.cls == "limbs"][:2]
    for k, o in enumerate(few):
        other = core[(7 * k + 11) % len(core)]
        for pos in range(width):
            out.append(("one-hot[%s@%d]" % (o.name, pos), pad([o.v if i == pos else 0 for i in range(width)])))
            out.append(("one-cold[%s,0@%d]" % (other.name, pos), pad([0 if i == pos else other.v for i in range(width)])))
    for sub, cnt in (("Fp", 1), ("Fp2", 2), ("Fp6", 6)):
        if cnt < width:
            for k, o in enumerate(core[::5]):
                out.append(("subfield-%s[%s]" % (sub, o.name), pad([core[(k + i) % len(core)].v if i else o.v for i in range(cnt)])))
    g = _Rng(seed + width)
    for k in range(n_drawn):
        out.append(("drawn[%d]" % k, pad([full[g.below(len(full))].v for _ in range(width)])))
    out.append(("zero", [0] * 12))
    out.append(("one", [1] + [0] * 11))
    return out


def load_searched():
    """the committed result of tests/golden/gen_adversarial.py"""
    with open(JSON_PATH) as f:
        return json.load(f)
