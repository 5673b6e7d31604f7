"""Limb-exact CPU model of the division-step inversion in zkvm_pairings_amd/csrc/zkp_coop.hip (f_inv): int32 limbs of 30 bits,
int64 accumulators, 37 batches of 30 steps (delta = 1 variant of Bernstein-Yang "safegcd").  `python3 tools/safegcd_model.py`
checks it against pow(x, -1, p) on random and edge values."""
import random
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
NL, W = 13, 30
M30 = (1 << W) - 1
NB = 37
PINV30 = pow(P, -1, 1 << W)
def s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x
def s64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x
def limbs(v):
    out = []
    for i in range(NL - 1):
        out.append(v & M30); v >>= W
    out.append(v); return out
def val(l): return sum(x << (W * i) for i, x in enumerate(l))
PL = limbs(P)
def divsteps30(eta, f0, g0):
    u, v, q, r = 1, 0, 0, 1
    f, g = f0 & 0xFFFFFFFF, g0 & 0xFFFFFFFF
    for _ in range(30):
        c1 = 0xFFFFFFFF if s32(eta) < 0 else 0
        c2 = (-(g & 1)) & 0xFFFFFFFF
        x = ((f ^ c1) - c1) & 0xFFFFFFFF; y = ((u ^ c1) - c1) & 0xFFFFFFFF; z = ((v ^ c1) - c1) & 0xFFFFFFFF
        g = (g + (x & c2)) & 0xFFFFFFFF; q = (q + (y & c2)) & 0xFFFFFFFF; r = (r + (z & c2)) & 0xFFFFFFFF
        c1 &= c2
        eta = ((eta ^ c1) - (c1 + 1)) & 0xFFFFFFFF
        f = (f + (g & c1)) & 0xFFFFFFFF; u = (u + (q & c1)) & 0xFFFFFFFF; v = (v + (r & c1)) & 0xFFFFFFFF
        g >>= 1; u = (u << 1) & 0xFFFFFFFF; v = (v << 1) & 0xFFFFFFFF
    return eta, (s32(u), s32(v), s32(q), s32(r))
def s16(x):
    x &= 0xFFFF
    return x - (1 << 16) if x >> 15 else x
def _h16(x):
    # one 16-bit half of a packed register: the kernel's v_pk_* result wraps, the true value must not
    assert s16(x) == x, "packed matrix half leaves int16 (%d)" % x
    return x
def mul24(a, b):
    # __mul24: the low 24 bits of each operand, sign-extended, multiplied; the low 32 bits of the product
    assert -(1 << 23) <= a < (1 << 23) and -(1 << 23) <= b < (1 << 23), "__mul24 operand leaves 24 signed bits (%d, %d)" % (a, b)
    return s32(a * b)
def divsteps30_packed(eta, f0, g0, stats=None):
    """sg::divsteps30 of zkp_coop.hip statement for statement: three runs of ten steps with the rows (u, v) and (q, r) as two 16-bit
    halves of one register each, the runs' matrices multiplied together with 24-bit multiplies that wrap mod 2^32.  stats (a dict)
    receives the largest entry magnitude of any run ("run_max") and of the batch ("batch_max")."""
    e = eta & 0xFFFFFFFF
    f, g = f0 & 0xFFFFFFFF, g0 & 0xFFFFFFFF
    U, V, Q, R = 1, 0, 0, 1
    for run in range(3):
        P_ = [1, 0]; T = [0, 1]
        for _ in range(10):
            c1 = 0xFFFFFFFF if s32(e) < 0 else 0
            c2 = (-(g & 1)) & 0xFFFFFFFF
            x = ((f ^ c1) - c1) & 0xFFFFFFFF
            m1 = -1 if c1 else 0; m2 = -1 if c2 else 0          # the same mask in both halves
            Y = [_h16((h ^ m1) - m1) for h in P_]
            g = (g + (x & c2)) & 0xFFFFFFFF
            T = [_h16(t + (y & m2)) for t, y in zip(T, Y)]
            c1 &= c2
            m1 = -1 if c1 else 0
            e = ((e ^ c1) - (c1 + 1)) & 0xFFFFFFFF
            f = (f + (g & c1)) & 0xFFFFFFFF
            P_ = [_h16(p + (t & m1)) for p, t in zip(P_, T)]
            g >>= 1
            P_ = [_h16(p + p) for p in P_]
        u2, v2, q2, r2 = P_[0], P_[1], T[0], T[1]
        if stats is not None:
            stats["run_max"] = max(stats.get("run_max", 0), abs(u2), abs(v2), abs(q2), abs(r2))
        if run == 0:
            U, V, Q, R = u2, v2, q2, r2
        else:
            nU = s32(mul24(u2, U) + mul24(v2, Q)); nV = s32(mul24(u2, V) + mul24(v2, R))
            nQ = s32(mul24(q2, U) + mul24(r2, Q)); nR = s32(mul24(q2, V) + mul24(r2, R))
            U, V, Q, R = nU, nV, nQ, nR
    if stats is not None:
        stats["batch_max"] = max(stats.get("batch_max", 0), abs(U), abs(V), abs(Q), abs(R))
    return e, (U, V, Q, R)
def update_fg(f, g, t):
    u, v, q, r = t
    cf = s64(u * f[0] + v * g[0]); cg = s64(q * f[0] + r * g[0])
    assert cf & M30 == 0 and cg & M30 == 0
    cf >>= W; cg >>= W
    for i in range(1, NL):
        cf = s64(cf + u * f[i] + v * g[i]); cg = s64(cg + q * f[i] + r * g[i])
        f[i - 1] = cf & M30; g[i - 1] = cg & M30
        cf >>= W; cg >>= W
    f[NL - 1] = s32(cf); g[NL - 1] = s32(cg)
    assert f[NL-1] == cf and g[NL-1] == cg
def update_de(d, e, t):
    u, v, q, r = t
    sd = -1 if d[NL - 1] < 0 else 0
    se = -1 if e[NL - 1] < 0 else 0
    md = (u & sd) + (v & se); me = (q & sd) + (r & se)
    cd = s64(u * d[0] + v * e[0]); ce = s64(q * d[0] + r * e[0])
    md -= (PINV30 * (cd & 0xFFFFFFFF) + md) & M30
    me -= (PINV30 * (ce & 0xFFFFFFFF) + me) & M30
    md = s32(md); me = s32(me)
    cd = s64(cd + PL[0] * md); ce = s64(ce + PL[0] * me)
    assert cd & M30 == 0 and ce & M30 == 0
    cd >>= W; ce >>= W
    for i in range(1, NL):
        cd = s64(cd + u * d[i] + v * e[i] + PL[i] * md); ce = s64(ce + q * d[i] + r * e[i] + PL[i] * me)
        d[i - 1] = cd & M30; e[i - 1] = ce & M30
        cd >>= W; ce >>= W
    d[NL - 1] = s32(cd); e[NL - 1] = s32(ce)
    assert d[NL-1] == cd and e[NL-1] == ce
def normalize(r, sign):
    # r in (-2p, p); sign < 0 -> negate.  result in [0, p)
    add = -1 if r[NL - 1] < 0 else 0
    neg = -1 if sign < 0 else 0
    c = 0
    for i in range(NL):
        x = r[i] + (PL[i] & add)
        x = (x ^ neg) - neg
        x += c
        if i < NL - 1:
            r[i] = x & M30; c = x >> W
        else:
            r[i] = x
    add = -1 if r[NL - 1] < 0 else 0
    c = 0
    for i in range(NL):
        x = r[i] + (PL[i] & add) + c
        if i < NL - 1:
            r[i] = x & M30; c = x >> W
        else:
            r[i] = x
    return r
def inv(x, packed=False, trace=None):
    """x^-1 mod p (0 for 0) through 37 batches; packed selects the kernel's packed formulation of a batch.  trace (a dict) receives
    "lows": the (eta, f[0], g[0]) every batch started from, "batches": batches until g == 0, "entry_max" / "run_max": the largest
    matrix entry of a batch / of a run of ten steps (packed only), "de_hi" / "de_lo": the extremes of d and e as multiples of p."""
    step = divsteps30_packed if packed else divsteps30
    f = list(PL); g = limbs(x); d = [0] * NL; e = [1] + [0] * (NL - 1)
    eta = -1
    for it in range(NB):
        if trace is not None:
            trace.setdefault("lows", []).append((s32(eta), f[0], g[0]))
        if packed:
            eta, t = step(eta, f[0], g[0], trace)
        else:
            eta, t = step(eta, f[0], g[0])
        update_de(d, e, t)
        update_fg(f, g, t)
        vd, ve = val(d), val(e)
        assert -2 * P < vd < P and -2 * P < ve < P, (vd / P, ve / P)
        if trace is not None:
            trace["entry_max"] = max(trace.get("entry_max", 0), *(abs(c) for c in t))
            trace["de_hi"] = max(trace.get("de_hi", 0.0), vd / P, ve / P)
            trace["de_lo"] = min(trace.get("de_lo", 0.0), vd / P, ve / P)
            if "batches" not in trace and val(g) == 0:
                trace["batches"] = it + 1
    assert val(g) == 0 and val(f) in ((1, -1) if x else (P, -P))
    r = normalize(d, f[NL - 1])
    return val(r)
def selftest(n=2000, seed=7):
    rng = random.Random(seed)
    for i in range(n):
        x = rng.randrange(1, P)
        assert inv(x) == pow(x, -1, P), i
        if i % 8 == 0:
            assert inv(x, packed=True) == pow(x, -1, P), i
    for x in (1, 2, 3, P - 1, P - 2, (P + 1) // 2, 1 << 380, (1 << 381) % P):
        assert inv(x) == pow(x, -1, P)
        assert inv(x, packed=True) == pow(x, -1, P)
    assert inv(0) == 0 and inv(0, packed=True) == 0
    return True


if __name__ == "__main__":
    selftest()
    print("limb model ok: 2000 random and the edge values agree with pow(x, -1, p)")
    print("PINV30", PINV30, "PL", PL)
