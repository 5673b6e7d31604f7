"""The bucket MSM at every shape its planner picks, and scalar multiplication at its edges, on one MI355X (run with -m gpu).

- Every window width c = 2..16 at both ends of its range (tests/msm_shapes.py, whose plans tests/test_msm_cpu.py proves on the CPU),
  by construction: bases drawn from a pool of [a_j]G, so each sum is [sum k_i a_i mod r]G, one oracle multiplication.  The scalars
  mix uniform 256-bit values with a family built window by window from the raw digits where the signed recoding turns.
- Every sum of a multi-pass call, with infinity flags at the first and last term of every pass: the steering scalar of each sum is
  solved for so that the sum hits a table of oracle points.
- Bases outside the prime-order subgroup (order-3 and cofactor points, their negations, duplicates) against the oracle's sum of
  multiples, so buckets, running sums and the Horner step meet doublings and P + (-P).
- zkp_g*_mul_batch on both kernel families at scalars around r, 2r and 2^256, on subgroup and non-subgroup bases, stride 0 and not.
- zkp_msm_profile_dev against the plain call.
Expected values come from the oracle (tests/oracle_lib.py) or from the construction of the inputs - never from the library under
test.  Every result is compared bit for bit; the identity is (0, 1) with its flag set."""
import math
import random

import numpy as np
import pytest

import bls12_381_model as bm
import msm_shapes as ms
import oracle_lib as o
from test_gpu_group import _assert_same, _cofactor_points, _gen, _neg, _oadd, _omul, _sc

pytestmark = pytest.mark.gpu
R = bm.R_ORDER
COLS = {1: 12, 2: 24}
POOL = 256                     # distinct bases [a_j]G the constructions draw from
TOP = (1 << 256) - 1


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=["thread", "coop"])
def keng(request, eng):
    """the same engine with each scalar-multiplication kernel family selected (jac_mul of zkp_field.hpp / k_g*_mul28)"""
    from zkvm_pairings_amd import _lib
    try:
        eng.set_kernel(request.param)
    except _lib.ZkpError:
        pytest.skip("kernel family %s not available in this build" % request.param)
    yield eng
    eng.set_kernel("auto")


@pytest.fixture(scope="module")
def pools():
    """per group: POOL bases [a_j]G with a_j uniform in [1, r), multiplied by the oracle"""
    out = {}
    for which in (1, 2):
        rng = random.Random(0x9001 + which)
        a = [rng.randrange(1, R) for _ in range(POOL)]
        out[which] = (_omul_many(which, np.tile(_gen(which), (POOL, 1)), a)[0], a)
    return out


def _msm(eng, which):
    return eng.g1_msm if which == 1 else eng.g2_msm


def _ints_to_scalars(ks):
    return np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), dtype=np.uint64).reshape(-1, 4).copy()


def _scalars_to_ints(sc):
    b = np.ascontiguousarray(sc, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _identity(which):
    ident = np.zeros(COLS[which], dtype=np.uint64)
    ident[6 * which] = 1
    return ident


def _omul_many(which, pts, ks):
    """[k_i] pts_i by the oracle on 16 threads -> (points, infinity flags); the oracle writes the identity as (0, 1), which is on
    neither curve"""
    mulb = o.g1_mul_batch if which == 1 else o.g2_mul_batch
    out = mulb(np.ascontiguousarray(pts, dtype=np.uint64), _sc(list(ks)), nthreads=16)
    return out, np.all(out == _identity(which), axis=1).astype(np.uint8)


def _oracle_sums(which, pts, inf, ks, m, n_msm, shared):
    """the oracle's sum of multiples of every segment: the multiples on 16 threads, then affine additions"""
    tp = np.tile(pts, (n_msm, 1)) if shared else pts
    ti = np.tile(inf, n_msm) if shared else inf
    mul, mi = _omul_many(which, tp, ks)
    out = []
    for j in range(n_msm):
        acc, ai = _identity(which), 1
        for i in range(j * m, (j + 1) * m):
            if not ti[i]:
                acc, ai = _oadd(which, acc, ai, mul[i], int(mi[i]))
        out.append((acc, ai))
    return out


def _family(c, count, rng):
    """scalars built window by window (c bits each, truncated to 256 bits) from the raw window values where the signed recoding
    turns: 0, 1, 2^(c-1) - 1, 2^(c-1), 2^(c-1) + 1 (negated, carries into the next window), 2^c - 1.  First every window one value
    (2^c - 1 throughout is an all-maximal carry chain, 2^256 - 1), then the six values rotated, then random picks; many are >= r."""
    h = 1 << (c - 1)
    vals = [0, 1, h - 1, h, h + 1, (1 << c) - 1]
    nw = 256 // c + 1
    build = lambda ds: sum(d << (c * w) for w, d in enumerate(ds)) & TOP
    out = [build([v] * nw) for v in vals]
    out += [build([vals[(w + i) % len(vals)] for w in range(nw)]) for i in range(len(vals))]
    out += [build([vals[i], vals[j]] * nw) for i in range(len(vals)) for j in range(len(vals)) if i != j]
    while len(out) < count:
        out.append(build([rng.choice(vals) for _ in range(nw)]))
    return out[:count]


def _scalars(rnp, rng, n, c):
    """n scalars: uniform 256-bit values, with the digit family of width c at random places (about half of them in small calls)"""
    sc = np.frombuffer(rnp.bytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
    fam = _family(c, min(256, (n + 1) // 2), rng)
    sc[rnp.integers(0, n, len(fam))] = _ints_to_scalars(fam)
    return sc


def _class_sums(sc, term_cls, m, n_msm, a):
    """per segment sum_i k_i a_(cls_i) mod r without a Python loop over the terms: sums of the scalars' 16-bit limbs per (segment,
    class) by bincount - exact in float64, at most 2^24 terms of 16 bits - then one big-integer combination per class and limb"""
    n = sc.shape[0]
    key = (np.arange(n, dtype=np.int64) // m) * POOL + term_cls
    l16 = np.ascontiguousarray(sc, dtype=np.uint64).view(np.uint16).reshape(n, 16)
    sums = np.stack([np.bincount(key, weights=l16[:, li].astype(np.float64), minlength=n_msm * POOL) for li in range(16)], axis=1)
    assert sums.max() < 2.0 ** 53
    sums = sums.astype(np.int64).reshape(n_msm, POOL, 16)
    out = []
    for j in range(n_msm):
        tot = 0
        for li in range(16):
            col = sums[j, :, li]
            tot += sum(a[i] * int(col[i]) for i in np.nonzero(col)[0]) << (16 * li)
        out.append(tot % R)
    return out


def _sid(s):
    return "m%d-n%d%s" % (s.m, s.n_msm, "-shared" if s.shared else "")


# ------------------------------------------------------------------------------------------------------------------- every width
@pytest.mark.parametrize("which,shape", [pytest.param(w, s, id="g%d-c%d-%s" % (w, s.c, _sid(s))) for s in ms.WIDTHS for w in s.groups])
def test_msm_every_window_width_by_construction(eng, pools, which, shape):
    pool, a = pools[which]
    seed = shape.m * 131 + shape.n_msm * 7 + which
    rng, rnp = random.Random(seed), np.random.default_rng(seed)
    m, n = shape.m, shape.n_msm
    cls = rnp.integers(0, POOL, m if shape.shared else m * n)
    sc = _scalars(rnp, rng, m * n, shape.c)
    got, gi = _msm(eng, which)(pool[cls], sc, n, None, shape.shared)
    want = _class_sums(sc, np.tile(cls, n) if shape.shared else cls, m, n, a)
    w, wi = _omul_many(which, np.tile(_gen(which), (n, 1)), want)
    for j in range(n):
        _assert_same(which, got[j], int(gi[j]), w[j], int(wi[j]))


# ------------------------------------------------------------------------------------------------------------------- every pass
@pytest.mark.parametrize("which,shape", [pytest.param(w, s, id="g%d-%s" % (w, _sid(s))) for s in ms.PASSES for w in s.groups])
def test_msm_every_sum_of_a_multi_pass_call(eng, pools, which, shape):
    """each sum's last live term is solved for so that the sum is [t_j]G, t_j from a table of 64 oracle points whose entry 0 is the
    identity (also reached by cancellation); infinity flags fall at random, on the first and last term of every pass, and on whole
    segments (non-shared), or on one shared base"""
    pool, a = pools[which]
    m, n, segs = shape.m, shape.n_msm, shape.segs
    seed = 0x9A55 + m * 17 + which + 2 * shape.shared
    rng, rnp = random.Random(seed), np.random.default_rng(seed)
    n_pts = m if shape.shared else m * n
    cls = rnp.integers(0, POOL, n_pts)
    inf = np.zeros(n_pts, dtype=np.uint8)
    if shape.shared:
        inf[m // 2] = 1
    else:
        inf[rnp.integers(0, n_pts, n_pts // 16)] = 1
        for p in range(shape.passes):
            inf[p * segs * m] = inf[min(n, (p + 1) * segs) * m - 1] = 1
    term_cls = np.tile(cls, n) if shape.shared else cls
    term_inf = np.tile(inf, n) if shape.shared else inf
    t_val = [0] + [rng.randrange(1, R) for _ in range(63)]
    table = _omul_many(which, np.tile(_gen(which), (64, 1)), t_val)[0]
    t_idx = rnp.integers(0, 64, n)
    ks = _scalars_to_ints(np.frombuffer(rnp.bytes(32 * m * n), dtype=np.uint64).reshape(-1, 4))
    inv = [pow(x, -1, R) for x in a]
    cl, fl = term_cls.tolist(), term_inf.tolist()
    for j in range(n):
        live = [i for i in range(j * m, j * m + m) if not fl[i]]
        if not live:
            t_idx[j] = 0
            continue
        st = live[-1]
        rest = sum(ks[i] * a[cl[i]] for i in live[:-1])
        k = (t_val[t_idx[j]] - rest) * inv[cl[st]] % R
        ks[st] = k + R * rng.randrange((TOP - k) // R + 1)
    got, gi = _msm(eng, which)(pool[cls], _ints_to_scalars(ks), n, inf, shape.shared)
    want, want_inf = table[t_idx], (t_idx == 0).astype(np.uint8)
    bad = np.nonzero(np.any(got != want, axis=1) | (gi != want_inf))[0]
    assert bad.size == 0, "%d of %d sums differ, first %d (pass %d)" % (bad.size, n, bad[0], bad[0] // segs)


# ------------------------------------------------------------------------------------------------------------------- outside the subgroup
@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("m,n_msm,shared", [(5, 96, False), (16, 40, False), (13, 32, True)])
def test_msm_points_outside_the_subgroup(eng, model_vectors, which, m, n_msm, shared):
    cand = _cofactor_points(model_vectors, which)
    cand = cand + [_neg(which, p) for p in cand]
    rng = random.Random(0x0DD + 100 * m + which + shared)
    n_pts = m if shared else m * n_msm
    pick = [rng.randrange(len(cand)) for _ in range(n_pts)]
    if not shared:
        for j in range(0, n_msm, 4):                                    # one base (and its negation) throughout: the buckets double
            pick[j * m:(j + 1) * m] = [pick[j * m]] * m
    pts = np.stack([cand[i] for i in pick])
    if not shared:
        half = len(cand) // 2
        for j in range(0, n_msm, 8):                                    # every other term negated: P + (-P) in the buckets
            for i in range(j * m + 1, (j + 1) * m, 2):
                pts[i] = cand[(pick[i] + half) % len(cand)]
    inf = np.array([rng.random() < 0.08 for _ in range(n_pts)], dtype=np.uint8)
    small = [1, 2, 3, 4, 5, 6, 9, 12]
    edge = [0, 1, R - 1, R, R + 1, R + 2, 2 * R, 1 << 255, TOP, (1 << 256) - R]
    ks = []
    for j in range(n_msm):
        kind = j % 3
        for _ in range(m):
            if kind == 0:
                ks.append(rng.getrandbits(256))
            elif kind == 1:
                ks.append(rng.choice(small))
            else:
                ks.append(rng.choice(edge + small) if rng.random() < 0.5 else rng.getrandbits(256))
    got, gi = _msm(eng, which)(pts, _sc(ks), n_msm, inf, shared)
    for j, (w, wi) in enumerate(_oracle_sums(which, pts, inf, ks, m, n_msm, shared)):
        _assert_same(which, got[j], int(gi[j]), w, wi)


# ------------------------------------------------------------------------------------------------------------------- scalar multiplication
MUL_EDGE = [R - 1, R, R + 1, R + 2, 2 * R - 1, 2 * R, 2 * R + 1, 2 * R + 4, 2 * R + 5, 1 << 255, TOP, (1 << 256) - R, 0, 1, 2, 3]


@pytest.mark.parametrize("which", [1, 2])
def test_scalar_mul_edge_scalars_on_both_kernel_families(keng, model_vectors, which):
    """scalars at and beyond r (k = r + 2 leaves P in the accumulator before the last mixed addition, 2r + 4 and 2r + 5 one bit
    earlier) on subgroup bases and on bases outside the subgroup, one base for all scalars (stride 0) and one base per scalar"""
    rng = random.Random(0x5CA1A + which)
    sub = [_gen(which), _omul(which, _gen(which), rng.randrange(1, R))[0]]
    out = _cofactor_points(model_vectors, which)
    bases = sub + out + [_neg(which, p) for p in out[:2]]
    ks = MUL_EDGE + [rng.getrandbits(256) for _ in range(8)]
    mul = keng.g1_mul if which == 1 else keng.g2_mul
    pb = np.stack([b for b in bases for _ in ks])
    w, wi = _omul_many(which, pb, ks * len(bases))
    nk = len(ks)
    for bi, b in enumerate(bases):                                     # stride 0
        got, gi = mul(b, _sc(ks))
        for i in range(nk):
            _assert_same(which, got[i], int(gi[i]), w[bi * nk + i], int(wi[bi * nk + i]))
    got, gi = mul(pb, _sc(ks * len(bases)))                            # stride 12 / 24
    for i in range(len(pb)):
        _assert_same(which, got[i], int(gi[i]), w[i], int(wi[i]))


# ------------------------------------------------------------------------------------------------------------------- profile hook
@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("shape", ms.PROFILE, ids=_sid)
def test_msm_profile_gives_the_plain_calls_bytes(eng, pools, which, shape):
    import torch
    pool, _ = pools[which]
    rnp = np.random.default_rng(0x9F0 + which + shape.m)
    m, n = shape.m, shape.n_msm
    pts = pool[rnp.integers(0, POOL, m if shape.shared else m * n)]
    sc = np.frombuffer(rnp.bytes(32 * m * n), dtype=np.uint64).reshape(-1, 4).copy()
    want, wi = _msm(eng, which)(pts, sc, n, None, shape.shared)
    dev = torch.device("cuda", 0)
    tb = torch.from_numpy(pts.view(np.int64)).to(dev)
    ts = torch.from_numpy(sc.view(np.int64)).to(dev)
    out, oi, phase = eng.msm_profile(which, tb, ts, n, shape.shared)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want) and np.array_equal(oi.cpu().numpy(), wi)
    assert len(phase) == 6 and all(math.isfinite(x) and x >= 0 for x in phase), phase
    assert sum(phase) > 0
