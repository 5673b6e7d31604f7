"""The table of capturable device-pointer entry points (helper of test_gpu_graph_replay.py, test_gpu_call_order.py and
test_replay_cases_cpu.py; not a test module).  One Case per entry point and shape: the C names it reaches, the engine method, and a
builder that returns three input sets A, B, C of identical shapes (host arrays, loaded into resident tensors by the tests) with the
expected output bytes of each.  Expected values come, in this order, from Python integers (everything in Fr), from the construction of
the inputs (verdicts, status bytes), or from the CPU oracle (tests/oracle_lib.py: pairings and group operations - every synthetic point
is [e] G with a known exponent e, so a group result is one oracle multiplication of the generator) - never from the library under test.
The inputs themselves are made through a second engine that never captures (`h`, host-pointer calls)."""
import random

import numpy as np

import bls12_381_model as bm
import compressed_model as cm
import oracle_lib as o

P, R = bm.P, bm.R_ORDER
Z2 = bm.BLS_X ** 2
M64 = (1 << 64) - 1
COLS = {1: 12, 2: 24}

# ------------------------------------------------------------------------------------------------------------------- exclusions
EXCLUDED = {
    "zkp_time_pairing_dev": "measurement: times launches with events on the context's own stream and waits for them on the host",
    "zkp_profile_pairing_dev": "measurement: brackets every launch with events and synchronises on the host",
    "zkp_msm_profile_dev": "measurement: synchronises between the MSM phases to time them",
    "zkp_clock_probe_dev": "measurement: a spin kernel for another stream, its result depends on the clocks, not on its inputs",
    "zkp_take_validation_status_dev": "waits for the stream and reads the validation word back: a host synchronisation by contract",
    "zkp_and_allreduce_dev": "needs an RCCL communicator; the two-rank tests (test_dist_gloo.py) own it",
    "zkp_pairing_check_batch_allreduce_dev": "needs an RCCL communicator; the two-rank tests own it",
    "zkp_pairing_gt_check_batch_allreduce_dev": "needs an RCCL communicator; the two-rank tests own it",
    "zkp_points_check_batch_allreduce_dev": "needs an RCCL communicator; the two-rank tests own it",
}


# ------------------------------------------------------------------------------------------------------------------- small helpers
def fr_rows(ints):
    """Python integers (below 2^256) -> (n, 4) uint64"""
    return np.array([[(int(v) >> (64 * i)) & M64 for i in range(4)] for v in ints], dtype=np.uint64).reshape(len(ints), 4)


def _sc(ints):
    return fr_rows([k % R for k in ints])


def _gen(which):
    from zkvm_pairings_amd import synthetic
    return synthetic.G1_GENERATOR if which == 1 else synthetic.G2_GENERATOR


def _g1(eng, ks):
    return eng.g1_mul(_gen(1), _sc(ks))[0]


def _g2(eng, ks):
    return eng.g2_mul(_gen(2), _sc(ks))[0]


def _pts(eng, which, ks):
    return (_g1 if which == 1 else _g2)(eng, ks)


def identity(which):
    p = np.zeros(COLS[which], dtype=np.uint64)
    p[6 * which] = 1
    return p


def expect_points(which, exps):
    """[e] G for each exponent by the oracle; e = 0 (mod r) is the identity, written (0, 1) with the flag set"""
    red = [e % R for e in exps]
    inf = np.array([1 if e == 0 else 0 for e in red], dtype=np.uint8)
    gen = o.g1_generator() if which == 1 else o.g2_generator()
    mul = o.g1_mul_batch if which == 1 else o.g2_mul_batch
    out = mul(np.tile(gen, (len(red), 1)), fr_rows([e or 1 for e in red]), nthreads=16)
    out[inf == 1] = identity(which)
    return out, inf


def _ab(rng, n):
    return np.array([[rng.getrandbits(64) | 1, rng.getrandbits(64)] for _ in range(n)], dtype=np.uint64).reshape(n, 2)


def _i32(v):
    return np.array([int(v)], dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------- batch builders (RLC)
def free_checks(eng, rng, n, k, bad=(), zero_first=False):
    """n checks of k pairs ([x_j]G1, [y_j]G2) with sum x_j y_j = 0 (mod r); checks in `bad` get x_(k-1) + 1.  k = 1: the G1 point is
    the identity (flagged).  zero_first: the first pair of every check has x = 0, flagged as infinity."""
    xs, ys, inf1 = [], [], np.zeros(n * k, dtype=np.uint8)
    for c in range(n):
        x = [rng.randrange(1, R) for _ in range(k)]
        y = [rng.randrange(1, R) for _ in range(k)]
        if zero_first or k == 1:
            x[0] = 0
            inf1[c * k] = 1
        if k > 1:
            x[k - 1] = (-sum(x[j] * y[j] for j in range(k - 1)) * pow(y[k - 1], -1, R)) % R
        if c in bad:
            x[k - 1] = (x[k - 1] + 1) % R
            if k == 1:
                inf1[c * k] = 0
        xs += x
        ys += y
    return _g1(eng, xs), _g2(eng, ys), inf1


def groth_checks(eng, rng, n, s2=3, bad=(), inf_col=False, inf_fixed=False):
    """e(A, B) prod_j e(C_j, D_j) = 1: a b + sum c_j d_j = 0, D_j fixed.  inf_col: C_1 of every check is the identity (c_1 = 0);
    inf_fixed: D_2 is the identity (d_2 = 0, C_2 arbitrary)."""
    d = [rng.randrange(1, R) for _ in range(s2)]
    if inf_fixed:
        d[2] = 0
    av, bv, cv = [], [], []
    ci = np.zeros(n * s2, dtype=np.uint8)
    for c in range(n):
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        cc = [rng.randrange(1, R) for _ in range(s2)]
        if inf_col:
            cc[1] = 0
            ci[c * s2 + 1] = 1
        cc[0] = (-(a * b + sum(cc[j] * d[j] for j in range(1, s2))) * pow(d[0], -1, R)) % R
        if c in bad:
            cc[0] = (cc[0] + 1) % R
        av.append(a)
        bv.append(b)
        cv += cc
    fixed = _g2(eng, d)
    fi = np.array([1 if x == 0 else 0 for x in d], dtype=np.uint8)
    return dict(g1=_g1(eng, av), g2=_g2(eng, bv), k=1, col_g1=_g1(eng, cv), col_inf1=ci if inf_col else None, fixed_g2=fixed,
                fixed_inf2=fi if inf_fixed else None)


# ------------------------------------------------------------------------------------------------------------------- the case record
class Case:
    """id; c_names: the `_dev` symbols one call reaches; method: the engine method; make(h, shape, seed) -> (sets, expected), three
    dicts of host arrays and three tuples of expected output arrays; run(eng, t, shape) -> the output tensors, t the dict of resident
    tensors; shape and the smaller shape of the eager call between the replays; nodes: 'kernel' or 'memset/copy' (module order)"""

    def __init__(self, id, c_names, method, make, run, shape, small, nodes="kernel", run_host=None):
        self.id, self.c_names, self.method, self.make, self.run = id, tuple(c_names), method, make, run
        self.shape, self.small, self.nodes = shape, small, nodes
        self.run_host = run_host or run          # the same call on host arrays (the engine methods take either kind)

    def __repr__(self):
        return self.id


_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------------- pairing family
def pairing_sets(h, n, k, seed):
    """three sets of n checks of k pairs with the oracle's Miller values, Gt values and ok bytes.  A: every second check is the
    identity (k = 1: through an infinity flag, on either side), more flags on the others; B: every check is, but for a flag on the last
    pair; C: no flags at all (k > 1: only the last check fails)."""
    def build():
        rng = random.Random(seed * 1000 + n * 10 + k)
        out = []
        for s in range(3):
            xs, ys = [], []
            i1, i2 = np.zeros(n * k, dtype=np.uint8), np.zeros(n * k, dtype=np.uint8)
            for c in range(n):
                x = [rng.randrange(1, R) for _ in range(k)]
                y = [rng.randrange(1, R) for _ in range(k)]
                good = (c % 2 == 0, True, c != n - 1)[s]
                if k > 1:
                    x[k - 1] = (-sum(x[j] * y[j] for j in range(k - 1)) * pow(y[k - 1], -1, R) + (0 if good else 1)) % R
                elif good and s != 2:
                    (i1 if c % 4 == 0 else i2)[c] = 1         # one pair: the identity only through an infinity flag
                xs += x
                ys += y
            if s == 0 and k > 1:
                i1[k::2 * k] = 1                             # the first pair of every second check
            if s == 1 and k > 1 and n > 1:
                i2[n * k - 1] = 1
            g1, g2 = _g1(h, xs), _g2(h, ys)
            ml = o.multi_miller_loop_batch(g1, g2, n, k, i1, i2)
            gt = o.final_exponentiation_batch(ml)
            ok = (gt == o.fp12_one()[None]).all(axis=1).astype(np.uint8)          # the check's definition: Gt == Gt::identity()
            pg = o.pairing_batch(g1, g2, i1, i2, nthreads=16)
            out.append(dict(g1=g1, g2=g2, inf1=i1, inf2=i2, ml=ml, gt=gt, ok=ok, pairs_gt=pg))
        assert n == 1 or (out[0]["ok"].any() and not out[0]["ok"].all())
        return out
    return _cached(("pairing", n, k, seed), build)


_PIN = ("g1", "g2", "inf1", "inf2")


def _pairing_case(name, c_name, method, outputs, run):
    def make(h, shape, seed):
        d = pairing_sets(h, shape[0], shape[1], seed)
        return [{x: s[x] for x in _PIN} for s in d], [outputs(s) for s in d]
    return [Case("%s-n%d-k%d" % (name, n, k), [c_name], method, make, run, (n, k), (1, k)) for n, k in ((1, 1), (65, 1), (5, 3))]


def _fexp_make(h, shape, seed):
    d = pairing_sets(h, shape[0], shape[1], seed)
    return [dict(f=s["ml"]) for s in d], [(s["gt"],) for s in d]


def _gt_check_run(e, t, sh):
    import torch
    n, k = sh
    gt = torch.empty((n, 72), dtype=torch.int64, device=t["g1"].device)
    ok = torch.empty(n, dtype=torch.uint8, device=t["g1"].device)
    flag = torch.empty(1, dtype=torch.int32, device=t["g1"].device)
    e.pairing_gt_check(t["g1"], t["g2"], k, gt, ok, flag, t["inf1"], t["inf2"])
    return gt, ok, flag


PAIRING = (
    _pairing_case("pairing", "zkp_pairing_batch_dev", "pairing", lambda s: (s["pairs_gt"],),
                  lambda e, t, sh: (e.pairing(t["g1"], t["g2"], t["inf1"], t["inf2"]),))
    + _pairing_case("multi_miller_loop", "zkp_multi_miller_loop_batch_dev", "multi_miller_loop", lambda s: (s["ml"],),
                    lambda e, t, sh: (e.multi_miller_loop(t["g1"], t["g2"], sh[1], t["inf1"], t["inf2"]),))
    + [Case("final_exponentiation-n%d-k%d" % (n, k), ["zkp_final_exponentiation_batch_dev"], "final_exponentiation", _fexp_make,
            lambda e, t, sh: (e.final_exponentiation(t["f"]),), (n, k), (1, k)) for n, k in ((1, 1), (65, 1), (5, 3))]
    + _pairing_case("pairing_check", "zkp_pairing_check_batch_dev", "pairing_check", lambda s: (s["ok"], _i32(s["ok"].all())),
                    lambda e, t, sh: e.pairing_check(t["g1"], t["g2"], sh[1], t["inf1"], t["inf2"]))
    + _pairing_case("pairing_gt_check", "zkp_pairing_gt_check_batch_dev", "pairing_gt_check", lambda s: (s["gt"], s["ok"], _i32(s["ok"].all())),
                    _gt_check_run)
)


# ------------------------------------------------------------------------------------------------------------------- one product check
def product_sets(h, n, seed):
    """n pairs as ONE check.  A: the product is one (the unflagged pairs cancel; n = 1: the pair is flagged); B: the last pair is bad;
    C: the first pair is bad.  Infinity flags differ between the sets."""
    def build():
        rng = random.Random(seed * 1000 + n)
        out = []
        for s in range(3):
            x = [rng.randrange(1, R) for _ in range(n)]
            y = [rng.randrange(1, R) for _ in range(n)]
            i1, i2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
            if n == 1:
                i1[0] = 1 if s == 0 else 0
            else:
                if s == 0:
                    i1[1:n - 1:3] = 1
                elif s == 1:
                    i2[2:n - 1:4] = 1
                live = [j for j in range(n - 1) if not (i1[j] or i2[j])]
                x[n - 1] = -sum(x[j] * y[j] for j in live) * pow(y[n - 1], -1, R) % R
                if s == 1:
                    x[n - 1] = (x[n - 1] + 1) % R
                if s == 2:
                    x[0] = (x[0] + 1) % R
            g1, g2 = _g1(h, x), _g2(h, y)
            ml = o.multi_miller_loop_batch(g1, g2, 1, n, i1, i2)[0]
            gt = o.final_exponentiation_batch(ml)[0]
            one = bool((gt == o.fp12_one()).all())
            assert one == (s == 0)
            each = o.multi_miller_loop_batch(g1, g2, n, 1, i1, i2)
            prod = each[0].copy()
            for f in each[1:]:
                prod = o.fp12_mul(prod, f)
            assert np.array_equal(prod, ml)
            out.append(dict(g1=g1, g2=g2, inf1=i1, inf2=i2, ml=ml, gt=gt, one=one, each=each))
        return out
    return _cached(("product", n, seed), build)


def _product_case(name, c_name, method, inputs, outputs, run):
    def make(h, shape, seed):
        d = product_sets(h, shape[0], seed)
        return [inputs(s) for s in d], [outputs(s) for s in d]
    return [Case("%s-n%d" % (name, n), [c_name], method, make, run, (n,), (1,), "memset/copy") for n in (1, 9, 65)]


PRODUCT = (
    _product_case("miller_product", "zkp_miller_product_dev", "miller_product", lambda s: {x: s[x] for x in _PIN}, lambda s: (s["ml"],),
                  lambda e, t, sh: (e.miller_product(t["g1"], t["g2"], t["inf1"], t["inf2"]),))
    + _product_case("fp12_product", "zkp_fp12_product_dev", "fp12_product", lambda s: dict(f=s["each"]), lambda s: (s["ml"],),
                    lambda e, t, sh: (e.fp12_product(t["f"]),))
    + _product_case("pairing_product_check", "zkp_pairing_product_check_dev", "pairing_product_check", lambda s: {x: s[x] for x in _PIN},
                    lambda s: (s["gt"], _i32(s["one"])), lambda e, t, sh: e.pairing_product_check(t["g1"], t["g2"], t["inf1"], t["inf2"]))
)


# ------------------------------------------------------------------------------------------------------------------- group operations
def outside_subgroup(which):
    from zkvm_pairings_amd import configs
    return _cached(("outside", which), lambda: configs.curve_point_outside_subgroup(which)).copy()


def _valid_make(which):
    def make(h, shape, seed):
        n = shape[0]
        rng = random.Random(seed * 100 + which)
        sets, exp = [], []
        for s in range(3):
            pts = _pts(h, which, [rng.randrange(1, R) for _ in range(n)])
            inf = np.zeros(n, dtype=np.uint8)
            st = np.zeros(n, dtype=np.uint8)
            bad = [i for i in range(n) if (i % 5 == 4, False, True)[s]]
            for j, i in enumerate(bad):
                if j % 2:
                    pts[i], st[i] = outside_subgroup(which), 2
                else:
                    pts[i, 6 * which] ^= np.uint64(1)       # y + 1 or y - 1: off the curve
                    st[i] = 1
            if s < 2:
                inf[(s + 1)::7] = 1
                inf[st != 0] = 0
            sets.append(dict(pts=pts, inf=inf))
            exp.append((st,))
        return sets, exp
    return make


def _mul_make(which):
    def make(h, shape, seed):
        n = shape[0]
        rng = random.Random(seed * 100 + 10 + which)
        sets, exp = [], []
        for s in range(3):
            a = [rng.randrange(1, R) for _ in range(n)]
            k = [rng.getrandbits(256) for _ in range(n)]
            for j, v in enumerate((0, R, 1, R - 1, (1 << 256) - 1)):
                k[(j * 13 + 3 * s) % n] = v                  # zero and r give the identity: the flags move between the sets
            sets.append(dict(base=_pts(h, which, a), scalars=fr_rows(k)))
            exp.append(expect_points(which, [x * y for x, y in zip(a, k)]))
        return sets, exp
    return make


def _add_make(which):
    def make(h, shape, seed):
        n = shape[0]
        rng = random.Random(seed * 100 + 20 + which)
        sets, exp = [], []
        for s in range(3):
            a = [rng.randrange(1, R) for _ in range(n)]
            b = [rng.randrange(1, R) for _ in range(n)]
            ia, ib = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
            b[s % n] = a[s % n]                              # a doubling
            b[(s + 3) % n] = R - a[(s + 3) % n]              # P + (-P)
            if s < 2:
                ia[(5 + s)::9] = 1
                ib[(2 * s)::11] = 1
            sets.append(dict(a=_pts(h, which, a), b=_pts(h, which, b), inf_a=ia, inf_b=ib))
            exp.append(expect_points(which, [(0 if ia[i] else a[i]) + (0 if ib[i] else b[i]) for i in range(n)]))
        return sets, exp
    return make


def msm_sets(h, which, m, n_msm, shared, seed):
    rng = random.Random(seed * 100 + 30 + which + 7 * m + n_msm + (1000 if shared else 0))
    np_ = m if shared else m * n_msm
    sets, exp = [], []
    for s in range(3):
        a = [rng.randrange(1, R) for _ in range(np_)]
        k = [rng.getrandbits(256) for _ in range(m * n_msm)]
        inf = np.zeros(np_, dtype=np.uint8)
        if s == 0:
            inf[::5] = 1
            k[0] = 0
        elif s == 1:
            inf[np_ - 1] = 1
            k[len(k) - 1] = R
        sums = []
        for j in range(n_msm):
            base = 0 if shared else j * m
            sums.append(sum(k[j * m + i] * a[base + i] for i in range(m) if not inf[base + i]))
        sets.append(dict(points=_pts(h, which, a), inf=inf, scalars=fr_rows(k)))
        exp.append(expect_points(which, sums))
    return sets, exp


def _msm_cases():
    out = []
    for which in (1, 2):
        for m, n_msm, shared in ((1, 1, False), (127, 1, False), (65, 2, False), (65, 2, True), (1000, 3, True)):
            run = (lambda w: lambda e, t, sh: (e.g1_msm if w == 1 else e.g2_msm)(t["points"], t["scalars"], sh[1], t["inf"], sh[2]))(which)
            make = (lambda w: lambda h, shape, seed: msm_sets(h, w, shape[0], shape[1], shape[2], seed))(which)
            out.append(Case("g%d_msm-m%d-x%d%s" % (which, m, n_msm, "-shared" if shared else ""), ["zkp_g%d_msm_batch_dev" % which], "g%d_msm" % which,
                            make, run, (m, n_msm, shared), (1, n_msm, shared)))
    return out


def _endo_make(h, shape, seed):
    n = shape[0]
    rng = random.Random(seed * 100 + 40)
    sets, exp = [], []
    for s in range(3):
        x = [rng.randrange(1, R) for _ in range(n)]
        ab = _ab(rng, n)
        inf = np.zeros(n, dtype=np.uint8)
        for j, v in enumerate(((0, 0), (1, 0), (0, 1), (M64, M64))):
            ab[(j * 7 + s) % n] = v
        if s < 2:
            inf[(3 + s)::8] = 1
        sets.append(dict(base=_g1(h, x), inf=inf, ab=ab))
        exp.append(expect_points(1, [0 if inf[i] else (int(ab[i, 0]) + int(ab[i, 1]) * Z2) * x[i] for i in range(n)]))
    return sets, exp


def _two(which, name):
    return "zkp_g%d_%s_batch_dev" % (which, name)


GROUP = (
    [Case("g%d_is_valid-n65" % w, [_two(w, "is_valid")], "g%d_is_valid" % w, _valid_make(w),
          (lambda w: lambda e, t, sh: ((e.g1_is_valid if w == 1 else e.g2_is_valid)(t["pts"], t["inf"]),))(w), (65,), (3,)) for w in (1, 2)]
    + [Case("g%d_mul-n65" % w, [_two(w, "mul")], "g%d_mul" % w, _mul_make(w),
            (lambda w: lambda e, t, sh: (e.g1_mul if w == 1 else e.g2_mul)(t["base"], t["scalars"]))(w), (65,), (3,)) for w in (1, 2)]
    + [Case("g%d_add-n65" % w, [_two(w, "add")], "g%d_add" % w, _add_make(w),
            (lambda w: lambda e, t, sh: (e.g1_add if w == 1 else e.g2_add)(t["a"], t["b"], t["inf_a"], t["inf_b"]))(w), (65,), (5,)) for w in (1, 2)]
    + [Case("g1_mul_endo-n65", ["zkp_g1_mul_endo_batch_dev"], "g1_mul_endo", _endo_make,
            lambda e, t, sh: e.g1_mul_endo(t["base"], t["ab"], t["inf"]), (65,), (3,))]
    + _msm_cases()
)


# ------------------------------------------------------------------------------------------------------------------- Fr
FR_OPS = ("mul", "add", "sub", "neg", "square", "invert")


def fr_model(op, a, b):
    return {"mul": a * b % R, "add": (a + b) % R, "sub": (a - b) % R, "neg": -a % R, "square": a * a % R,
            "invert": pow(a, R - 2, R)}[op]


def _fr_vals(rng, n, s):
    v = [rng.randrange(R) for _ in range(n)]
    for j, x in enumerate((0, 1, R - 1, 2, (R + 1) // 2)):
        v[(j * 11 + 5 * s) % n] = x
    return v


def _fr_op_make(op):
    def make(h, shape, seed):
        rng = random.Random(seed * 100 + 50 + FR_OPS.index(op))
        sets, exp = [], []
        for s in range(3):
            a, b = _fr_vals(rng, shape[0], s), _fr_vals(rng, shape[0], s + 1)
            sets.append(dict(a=fr_rows(a), b=fr_rows(b)))
            exp.append((fr_rows([fr_model(op, x, y) for x, y in zip(a, b)]),))
        return sets, exp
    return make


def _wide_make(h, shape, seed):
    rng = random.Random(seed * 100 + 60)
    sets, exp = [], []
    for s in range(3):
        v = [rng.getrandbits(512) for _ in range(shape[0])]
        for j, x in enumerate((0, (1 << 512) - 1, R, R - 1, R << 256)):
            v[(j * 9 + s) % shape[0]] = x
        sets.append(dict(bytes=np.frombuffer(b"".join(x.to_bytes(64, "little") for x in v), dtype=np.uint8).reshape(-1, 64).copy()))
        exp.append((fr_rows([x % R for x in v]),))
    return sets, exp


def fold_sets(n, l, seed):
    rng = random.Random(seed * 100 + 70 + n + l)
    sets, exp = [], []
    for s in range(3):
        w = _fr_vals(rng, n, s)
        x = [[rng.randrange(R) for _ in range(l)] for _ in range(n)]
        if s == 2:
            x[n - 1] = [R - 1] * l
            w[n - 1] = R - 1
        sets.append(dict(w=fr_rows(w), x=fr_rows([v for row in x for v in row]).reshape(n, l, 4)))
        exp.append((fr_rows([sum(w[c] * x[c][i] for c in range(n)) % R for i in range(l)]), fr_rows([sum(w) % R]).reshape(4)))
    return sets, exp


def invert_sets(n, seed):
    """the zeros move: A none, B one in the last run of the last workgroup, C all"""
    rng = random.Random(seed * 100 + 80 + n)
    sets, exp = [], []
    for s in range(3):
        a = [rng.randrange(1, R) for _ in range(n)]
        if s == 1:
            a[n - 1] = 0
        if s == 2:
            a = [0] * n
        sets.append(dict(a=fr_rows(a)))
        exp.append((fr_rows([pow(x, R - 2, R) for x in a]),))
    return sets, exp


def eval_sets(log2_n, n_poly, bitrev, seed):
    """A: z inside the domain for polynomial 1 only; B: every z outside; C: every z inside, at indices 0, N/2 and N - 1"""
    from zkvm_pairings_amd import synthetic
    rng = random.Random(seed * 100 + 90 + log2_n + (50 if bitrev else 0))
    big_n = 1 << log2_n
    w = synthetic.fr_root_of_unity(log2_n)
    dom = [pow(w, i, R) for i in range(big_n)]
    domset = set(dom)
    sets, exp = [], []
    for s in range(3):
        ev = [[rng.randrange(R) for _ in range(big_n)] for _ in range(n_poly)]
        z = []
        for j in range(n_poly):
            v = rng.randrange(R)
            while v in domset:
                v = rng.randrange(R)
            z.append(v)
        if s == 0:
            z[1 % n_poly] = dom[(big_n // 3) % big_n]
        if s == 2:
            z = [dom[(0, big_n // 2, big_n - 1)[j % 3] % big_n] for j in range(n_poly)]
        sets.append(dict(evals=fr_rows([v for row in ev for v in row]).reshape(n_poly, big_n, 4), z=fr_rows(z)))
        exp.append((fr_rows([synthetic.barycentric_eval(ev[j], z[j], log2_n, bitrev) for j in range(n_poly)]),))
    return sets, exp


FR = (
    [Case("fr_op-%s-n65" % op, ["zkp_fr_op_batch_dev"], "fr_op", _fr_op_make(op), (lambda op: lambda e, t, sh: (e.fr_op(op, t["a"], t["b"]),))(op),
          (65,), (3,)) for op in FR_OPS]
    + [Case("fr_from_wide-n65", ["zkp_fr_from_wide_batch_dev"], "fr_from_wide", _wide_make, lambda e, t, sh: (e.fr_from_wide(t["bytes"]),), (65,), (3,))]
    + [Case("fr_fold-n%d-l%d" % (n, l), ["zkp_fr_fold_batch_dev"], "fr_fold", lambda h, shape, seed: fold_sets(shape[0], shape[1], seed),
            lambda e, t, sh: e.fr_fold(t["w"], t["x"]), (n, l), (3, 2)) for n, l in ((65, 3), (1000, 64))]
    + [Case("fr_invert-n%d" % n, ["zkp_fr_invert_batch_dev"], "fr_invert", lambda h, shape, seed: invert_sets(shape[0], seed),
            lambda e, t, sh: (e.fr_invert(t["a"]),), (n,), (3,)) for n in (5, 1025)]
    + [Case("fr_eval-log%d-x%d%s" % (lg, npoly, "-bitrev" if br else ""), ["zkp_fr_eval_batch_dev"], "fr_eval",
            lambda h, shape, seed: eval_sets(shape[0], shape[1], shape[2], seed),
            lambda e, t, sh: (e.fr_eval(t["evals"], t["z"], sh[0], sh[2]),), (lg, npoly, br), (0, 2, br))
       for lg, npoly, br in ((0, 3, False), (9, 3, False), (9, 3, True))]
)


# ------------------------------------------------------------------------------------------------------------------- codecs
def _fe(row, i):
    return sum(int(x) << (64 * j) for j, x in enumerate(row[6 * i:6 * i + 6]))


def encode_model(pt, which, inf=False):
    """uncompressed big-endian bytes of one wire-format point (G2: c1 before c0)"""
    if inf:
        return bytes([0x40]) + bytes(96 * which - 1)
    order = (0, 1) if which == 1 else (1, 0, 3, 2)
    return b"".join(_fe(pt, i).to_bytes(48, "big") for i in order)


def compress_model(pt, which, inf=False):
    if inf:
        return (cm.g1_compress if which == 1 else cm.g2_compress)(None)
    if which == 1:
        return cm.g1_compress((_fe(pt, 0), _fe(pt, 1)))
    return cm.g2_compress(((_fe(pt, 0), _fe(pt, 1)), (_fe(pt, 2), _fe(pt, 3))))


def _p_bytes():
    return P.to_bytes(48, "big")


def bad_string(which, compressed, kind, good, j=0):
    """(bytes, points-check status): a string that must be refused, made from the encoding `good` of a valid point.  kind 0: malformed
    flags (2), 1: a coordinate >= p (1), 2: not on the curve (3), 3: on the curve, outside the subgroup (4)"""
    from zkvm_pairings_amd import configs
    b = bytearray(good)
    if kind == 0:
        b[0] = (b[0] & 0x7F) if compressed else (b[0] | 0x80)
        return bytes(b), 2
    if kind == 1:
        b[:48] = _p_bytes()
        if compressed:
            b[0] |= 0x80
        return bytes(b), 1
    if kind == 2:
        if not compressed:
            b[-1] ^= 1
            return bytes(b), 3
        x = _cached(("no root", which), lambda: configs._x_not_on_curve(which, 4))[j % 4]
        raw = x.to_bytes(48, "big") if which == 1 else x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big")
        b = bytearray(raw)
        b[0] |= 0x80
        return bytes(b), 3
    pt = outside_subgroup(which)
    return (compress_model if compressed else encode_model)(pt, which), 4


def _rows_u8(strings):
    return np.frombuffer(b"".join(strings), dtype=np.uint8).reshape(len(strings), -1).copy()


def _encode_make(which, compressed):
    model = compress_model if compressed else encode_model

    def make(h, shape, seed):
        n = shape[0]
        rng = random.Random(seed * 100 + 110 + which + (2 if compressed else 0))
        sets, exp = [], []
        for s in range(3):
            pts = _pts(h, which, [rng.randrange(1, R) for _ in range(n)])
            inf = np.zeros(n, dtype=np.uint8)
            if s < 2:
                inf[(1 + 2 * s)::6] = 1
            sets.append(dict(pts=pts, inf=inf))
            exp.append((_rows_u8([model(pts[i], which, bool(inf[i])) for i in range(n)]),))
        return sets, exp
    return make


def _decode_make(which, compressed):
    """A: every fifth string is refused; B: all decode; C: all are refused.  Codec statuses: 0, 1 coordinate >= p, 2 malformed and,
    compressed only, 3 no square root; a refused point comes out as zeros, the identity as (0, 1) with the flag"""
    model = compress_model if compressed else encode_model

    def make(h, shape, seed):
        n = shape[0]
        rng = random.Random(seed * 100 + 120 + which + (2 if compressed else 0))
        sets, exp = [], []
        for s in range(3):
            pts = _pts(h, which, [rng.randrange(1, R) for _ in range(n)])
            inf = np.zeros(n, dtype=np.uint8)
            st = np.zeros(n, dtype=np.uint8)
            raw = []
            for i in range(n):
                if (i % 5 == 4, False, True)[s]:
                    kind = (i // 5 + i % 5) % (3 if compressed else 2)      # the codec's statuses 2, 1 and (compressed) 3
                    string, st[i] = bad_string(which, compressed, kind, model(pts[i], which), i)
                    pts[i] = 0
                elif s < 2 and i % 6 == 1 + s:
                    string, pts[i], inf[i] = model(None, which, True), identity(which), 1
                else:
                    string = model(pts[i], which)
                raw.append(string)
            sets.append(dict(bytes=_rows_u8(raw)))
            exp.append((pts, inf, st))
        return sets, exp
    return make


def _codec_cases():
    out = []
    for w in (1, 2):
        out.append(Case("g%d_encode-n65" % w, [_two(w, "encode")], "encode_points_dev", _encode_make(w, False),
                        (lambda w: lambda e, t, sh: (e.encode_points_dev(t["pts"], w, t["inf"]),))(w), (65,), (3,)))
        out.append(Case("g%d_decode-n65" % w, [_two(w, "decode")], "decode_points_dev", _decode_make(w, False),
                        (lambda w: lambda e, t, sh: e.decode_points_dev(t["bytes"], w))(w), (65,), (3,)))
        out.append(Case("g%d_compress-n65" % w, [_two(w, "compress")], "compress_points_dev", _encode_make(w, True),
                        (lambda w: lambda e, t, sh: (e.compress_points_dev(t["pts"], w, t["inf"]),))(w), (65,), (3,)))
        out.append(Case("g%d_decompress-n65" % w, [_two(w, "decompress")], "decompress_points_dev", _decode_make(w, True),
                        (lambda w: lambda e, t, sh: e.decompress_points_dev(t["bytes"], w))(w), (65,), (3,)))
    return out


CODEC = _codec_cases()


# ------------------------------------------------------------------------------------------------------------------- the points check
def _neg_g1(pt):
    q = pt.copy()
    q[6:] = o.to_limbs((P - _fe(pt, 1)) % P)
    return q


def points_check_sets(h, n, k, compressed, seed):
    """n checks of k pairs as byte strings.  Valid checks: k = 1: even checks have P = the infinity encoding (ok = 1), odd ones a random
    pair (ok = 0); k = 2: (P, Q), (-P, Q) (ok = 1), every third check (P, Q), (P, Q) (ok = 0).  A: every fifth point is refused (the
    four kinds of refusal in turn, on the G1 and G2 side in turn); B: every point valid; C: every G1 point is refused, so the compacted count is zero."""
    model = compress_model if compressed else encode_model
    rng = random.Random(seed * 100 + 130 + n + k + (5 if compressed else 0))
    sets, exp = [], []
    for s in range(3):
        g1, g2 = _g1(h, [rng.randrange(1, R) for _ in range(n * k)]), _g2(h, [rng.randrange(1, R) for _ in range(n * k)])
        b1, b2 = [], []
        st1, st2 = np.zeros(n * k, dtype=np.uint8), np.zeros(n * k, dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        for c in range(n):
            if k == 1:
                i = c
                ok[c] = 1 if c % 2 == 0 else 0
                b1.append(model(g1[i], 1, inf=(c % 2 == 0)))
                b2.append(model(g2[i], 2))
            else:
                i = 2 * c
                ok[c] = 0 if c % 3 == 2 else 1
                b1 += [model(g1[i], 1), model(g1[i] if c % 3 == 2 else _neg_g1(g1[i]), 1)]
                b2 += [model(g2[i], 2), model(g2[i], 2)]
        for i in range(n * k):
            if s == 1 or (s == 0 and i % 5 != 4) or False:
                continue
            side = 1 if s == 2 else 1 + (i // 5) % 2
            kind = (i // 10 + i) % 4
            if side == 1:
                b1[i], st1[i] = bad_string(1, compressed, kind, model(g1[i], 1), i)
            else:
                b2[i], st2[i] = bad_string(2, compressed, kind, model(g2[i], 2), i)
            ok[i // k] = 0
        sets.append(dict(b1=_rows_u8(b1), b2=_rows_u8(b2)))
        exp.append((st1, st2, ok, _i32(ok.all())))
    return sets, exp


def _points_run(compressed, k):
    def run(e, t, sh):
        import torch
        dev = t["b1"].device
        np_ = t["b1"].shape[0]
        st1 = torch.empty(np_, dtype=torch.uint8, device=dev)
        st2 = torch.empty(np_, dtype=torch.uint8, device=dev)
        ok = torch.empty(np_ // k, dtype=torch.uint8, device=dev)
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        (e.points_check_compressed if compressed else e.points_check)(t["b1"], t["b2"], k, st1, st2, ok, flag)
        return st1, st2, ok, flag
    return run


def _points_run_host(compressed):
    return lambda e, t, sh: (e.points_check_compressed if compressed else e.points_check)(t["b1"], t["b2"], sh[1])


POINTS = [Case("points_check%s-n%d-k%d" % ("_compressed" if comp else "", n, k),
               ["zkp_points_check_compressed_batch_dev" if comp else "zkp_points_check_batch_dev"],
               "points_check_compressed" if comp else "points_check",
               (lambda comp: lambda h, shape, seed: points_check_sets(h, shape[0], shape[1], comp, seed))(comp), _points_run(comp, k), (n, k), (3, k),
               "memset/copy", _points_run_host(comp)) for comp in (False, True) for n, k in ((321, 1), (64, 2))]


# ------------------------------------------------------------------------------------------------------------------- verdict calls
def rlc_sets(h, kind, n, seed):
    """kind 'groth': the Groth16 shape, three fixed-G2 columns without flags of the fixed points (the driver zeroes them);
    'groth_flags': the same with infinity flags on a column and a fixed point (the driver copies them); 'free': k = 3 free pairs.
    A: every check holds; B: the last check is bad; C: check 1 is bad."""
    rng = random.Random(seed * 100 + 140 + n + len(kind))
    sets, exp = [], []
    for s, bad in enumerate((set(), {n - 1}, {1})):
        if kind == "free":
            g1, g2, i1 = free_checks(h, rng, n, 3, bad=bad, zero_first=(s == 0))
            d = dict(g1=g1, g2=g2, inf1=i1)
        else:
            kw = groth_checks(h, rng, n, bad=bad, inf_col=(kind == "groth_flags"), inf_fixed=(kind == "groth_flags"))
            d = {x: v for x, v in kw.items() if isinstance(v, np.ndarray)}
        d["rand"] = _ab(rng, n)
        sets.append(d)
        exp.append((_i32(not bad),))
    return sets, exp


def _rlc_run(k):
    def run(e, t, sh):
        kw = {x: t[x] for x in ("inf1", "col_g1", "col_inf1", "fixed_g2", "fixed_inf2") if x in t}
        return (e.pairing_check_rlc(t["g1"], t["g2"], k, rand=t["rand"], **kw),)
    return run


def groth16_sets(h, n, l, seed, bads=None):
    from zkvm_pairings_amd import synthetic
    sets, exp = [], []
    for s, bad in enumerate(bads if bads is not None else ((), (n - 1,), (0,))):
        key, proofs, inputs = synthetic.groth16_instance(seed * 16 + s, n, l, bad=bad, engine=h)
        sets.append(dict(alpha=key[0], beta=key[1], gamma=key[2], delta=key[3], ic=key[4], a=proofs[0], b=proofs[1], c=proofs[2],
                         inputs=inputs, rand=_ab(random.Random(seed + s), n)))
        exp.append((_i32(not bad),))
    return sets, exp


def groth16_call(e, t):
    return e.groth16_verify_batch(t["alpha"], t["beta"], t["gamma"], t["delta"], t["ic"], t["a"], t["b"], t["c"], t["inputs"], rand=t["rand"])


def kzg_sets(h, n, seed, bads=None):
    from zkvm_pairings_amd import synthetic
    sets, exp = [], []
    for s, bad in enumerate(bads if bads is not None else ((), (n - 1,), (0,))):
        setup, c, z, y, proof = synthetic.kzg_instance(seed * 16 + s, n, bad=bad, engine=h)
        sets.append(dict(g1=setup[0], g2=setup[1], tau_g2=setup[2], c=c, z=z, y=y, proof=proof, rand=_ab(random.Random(seed + 8 + s), n)))
        exp.append((_i32(not bad),))
    return sets, exp


def kzg_call(e, t):
    return e.kzg_verify_batch(t["g1"], t["g2"], t["tau_g2"], t["c"], t["z"], t["y"], t["proof"], rand=t["rand"])


VERDICT = [
    Case("groth16-n5-l3", ["zkp_groth16_verify_batch_dev"], "groth16_verify_batch", lambda h, shape, seed: groth16_sets(h, shape[0], shape[1], seed),
         lambda e, t, sh: (groth16_call(e, t),), (5, 3), (2, 3), "memset/copy"),
    Case("kzg-n5", ["zkp_kzg_verify_batch_dev"], "kzg_verify_batch", lambda h, shape, seed: kzg_sets(h, shape[0], seed),
         lambda e, t, sh: (kzg_call(e, t),), (5,), (2,), "memset/copy"),
    Case("rlc-groth-n24", ["zkp_pairing_check_batch_rlc_dev"], "pairing_check_rlc", lambda h, shape, seed: rlc_sets(h, "groth", shape[0], seed),
         _rlc_run(1), (24,), (4,), "memset/copy"),
    Case("rlc-groth-flags-n24", ["zkp_pairing_check_batch_rlc_dev"], "pairing_check_rlc",
         lambda h, shape, seed: rlc_sets(h, "groth_flags", shape[0], seed), _rlc_run(1), (24,), (4,), "memset/copy"),
    Case("rlc-free-k3-n6", ["zkp_pairing_check_batch_rlc_dev"], "pairing_check_rlc", lambda h, shape, seed: rlc_sets(h, "free", shape[0], seed),
         _rlc_run(3), (6,), (2,), "memset/copy"),
]

# kernel-node-only graphs first; the cases whose captured paths hold memset or copy nodes last
CASES = sorted(PAIRING + GROUP + FR + CODEC + PRODUCT + VERDICT + POINTS, key=lambda c: c.nodes != "kernel")


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
