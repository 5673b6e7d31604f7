"""Field, tower and inversion kernels on adversarial operands (run with -m gpu on an MI355X): the pool of tests/adversarial.py and
the vectors tests/golden/gen_adversarial.py searched on the CPU models, through zkp_fp_op_batch (both limb cores), zkp_tower_op_batch
and zkp_final_exponentiation_batch (both kernel families) and the square roots.  Every result of every batch is compared - with
Python integers for the field operations, with the CPU oracle bit for bit for the tower (tests/test_adversarial_cpu.py pins the
oracle on the same operands first).  All inputs are canonical and inside the ABI's contract: the aim is wrong values."""
import numpy as np
import pytest

import adversarial as adv
import bls12_381_model as m
import compressed_model as cm
import oracle_lib as o
from test_gpu_parity import _decompress_model

pytestmark = pytest.mark.gpu

P = m.P
SEARCHED = adv.load_searched()
H = lambda s: int(s, 16)
ROTATIONS = (1, 7)          # 7: a prime that divides neither 5 (checks per wavefront of the step interpreter) nor 16 (k_ksq)


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=["thread", "coop"])
def keng(request, eng):
    """the same engine with each Miller / final-exponentiation / tower kernel family selected"""
    from zkvm_pairings_amd import _lib
    try:
        eng.set_kernel(request.param)
    except _lib.ZkpError:
        pytest.skip("kernel family %s not available in this build" % request.param)
    eng.family = request.param
    yield eng
    eng.set_kernel("auto")


def fp_arr(vals):
    """list of canonical ints -> (n, 6) uint64"""
    return np.frombuffer(b"".join(int(v).to_bytes(48, "little") for v in vals), dtype=np.uint64).reshape(-1, 6).copy()


def rec_arr(recs):
    """list of [12 ints] -> (n, 72) uint64"""
    return fp_arr([v for r in recs for v in r]).reshape(-1, 72)


def same(got, want, what, label):
    """plain array comparison; the message names what ran and the first record that differs"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    i = int(bad[0])
    show = lambda r: [hex(x) for x in o.arr_to_ints(r)] if r.ndim and r.size % 6 == 0 else r.tolist()      # records, or a flag
    raise AssertionError("%s: %d of %d results differ; first at index %d (%s)\n got  %s\n want %s" % (
        what, len(bad), len(got), i, label(i), show(got[i]), show(want[i])))


def searched_fp_ops():
    """Fp values of the search: the g values of the division-step targets, as themselves and as the R = 2^392 pre-images whose
    stored representative they are, and the distinct coefficients of the searched tower records"""
    r28 = pow(adv.R28, -1, P)
    out = []
    for d in SEARCHED["divsteps"]:
        g = H(d["g"])
        out.append(adv.Op("searched", "%s[g]" % d["label"], g))
        out.append(adv.Op("searched", "%s[g/R]" % d["label"], g * r28 % P))
    for v in SEARCHED["vectors"]:
        for k in ("a", "b"):
            for i, x in enumerate(v.get(k) or []):
                out.append(adv.Op("searched", "%s.%s[%d]" % (v["label"], k, i), H(x)))
    return adv._dedupe(out)


def multiples_of_2_30():
    """values whose low 30 / 60 / 90 bits are zero, and their R = 2^392 pre-images: as the g of f_inv they make whole batches of
    thirty "g even" steps, whose transition matrix has an entry of exactly 2^30"""
    r28 = pow(adv.R28, -1, P)
    g = adv._Rng(0x2E30)
    vals = []
    for sh in (30, 60, 90, 150, 360):
        for t in (1, 3, (1 << 20) - 1, g.below(1 << 300) | 1, g.below(P) | 1):
            vals.append(adv.Op("mult2^30", "%d*2^%d" % (t, sh), (t << sh) % (1 << 380)))
    vals = adv._dedupe([v for v in vals if v.v])
    return vals + adv.preimages(vals, adv.R28, "mult2^30/R28")


BIN = {"mul": lambda x, y: x * y % P, "add": lambda x, y: (x + y) % P, "sub": lambda x, y: (x - y) % P}
UN = {"neg": lambda x: (-x) % P, "square": lambda x: x * x % P, "invert": lambda x: pow(x, -1, P) if x else 0}


@pytest.mark.parametrize("core28", [False, True], ids=["core32", "core28"])
def test_fp_binary_ops_on_the_full_cross_product(eng, core28):
    """mul / add / sub on pool x pool (ends, limb boundaries, their Montgomery pre-images on both cores, the searched values): every
    pair, every result against Python integers"""
    ops = adv._dedupe(adv.cross_set() + searched_fp_ops() + multiples_of_2_30())
    xs = [op.v for op in ops]
    n = len(xs)
    base = fp_arr(xs)
    a, b = np.repeat(base, n, axis=0), np.tile(base, (n, 1))
    for name, fn in BIN.items():
        want = fp_arr([fn(x, y) for x in xs for y in xs])
        got = eng.fp_op(name, a, b, core28=core28)
        same(got, want, "fp %s core28=%s cross product" % (name, core28),
             lambda i: "a = %s:%s, b = %s:%s" % (ops[i // n].cls, ops[i // n].name, ops[i % n].cls, ops[i % n].name))


@pytest.mark.parametrize("core28", [False, True], ids=["core32", "core28"])
def test_fp_binary_ops_powers_of_two_and_targeted_pairs(eng, core28):
    """class pow2 (and its pre-images) against a subset of the pool in both orders, and the pairs built to land the result on
    p - 1, p, p + 1 / -1, 0, 1 / 0, 1, p - 1, 2, (p + 1) / 2 before canonicalisation"""
    p2 = adv.powers_of_two()
    big = adv._dedupe(p2 + adv.preimages(p2, adv.R28, "pre28") + adv.preimages(p2, adv.R32, "pre32"))
    sub = adv.ends() + [op for op in adv.core_values() if op.cls == "limbs"][:16]
    pairs = [(x, y) for x in big for y in sub] + [(y, x) for x in big for y in sub]
    labels = ["a = %s:%s, b = %s:%s" % (x.cls, x.name, y.cls, y.name) for x, y in pairs]
    av, bv = [x.v for x, _ in pairs], [y.v for _, y in pairs]
    for tname, lst in adv.targeted_pairs().items():
        for nm, x, y in lst:
            av.append(x)
            bv.append(y)
            labels.append("pairs:%s from %s" % (tname, nm))
    a, b = fp_arr(av), fp_arr(bv)
    for name, fn in BIN.items():
        want = fp_arr([fn(x, y) for x, y in zip(av, bv)])
        same(eng.fp_op(name, a, b, core28=core28), want, "fp %s core28=%s" % (name, core28), lambda i: labels[i])


@pytest.mark.parametrize("core28", [False, True], ids=["core32", "core28"])
def test_fp_unary_ops_on_the_whole_pool(eng, core28):
    """neg / square / invert on every value of the pool.  For invert on the 28-bit core the R = 2^392 pre-images are the point: the
    division steps of f_inv start from g = the canonical stored representative = the structured value (2^k: long runs of "g even"
    steps; multiples of 2^30: matrix entries of exactly 2^30; the searched values: most batches, d and e at their bounds)"""
    ops = adv._dedupe(adv.pool() + searched_fp_ops() + multiples_of_2_30())
    xs = [op.v for op in ops]
    a = fp_arr(xs)
    for name, fn in UN.items():
        want = fp_arr([fn(x) for x in xs])
        same(eng.fp_op(name, a, core28=core28), want, "fp %s core28=%s" % (name, core28), lambda i: "%s:%s" % (ops[i].cls, ops[i].name))


# ---------------------------------------------------------------------------------------------------------------- tower
def _z(width, r):
    out = np.zeros(72, dtype=np.uint64)
    if r is not None:
        out[:width] = r
    return out


# op -> (Fp coefficients of a, of b, program names of the searched vectors that fit, oracle on (a, b) records of 72 u64)
TOWER = {
    "fp2_mul": (2, 2, ("tower:fp2_mul",), lambda a, b: _z(12, o.fp2_mul(a[:12], b[:12]))),
    "fp2_square": (2, 0, ("tower:fp2_sqr",), lambda a, b: _z(12, o.fp2_square(a[:12]))),
    "fp6_mul": (6, 6, ("tower:fp6_mul",), lambda a, b: _z(36, o.fp6_mul(a[:36], b[:36]))),
    "fp6_square": (6, 0, ("tower:fp6_sqr",), lambda a, b: _z(36, o.fp6_square(a[:36]))),
    "fp6_frobenius": (6, 0, (), lambda a, b: _z(36, o.fp6_frobenius_map(a[:36]))),
    "fp12_mul": (12, 12, ("tower:fp12_mul",), lambda a, b: o.fp12_mul(a, b)),
    "fp12_square": (12, 0, ("tower:fp12_sqr", "ksq", "kdec"), lambda a, b: o.fp12_square(a)),
    "fp12_mul_by_014": (12, 6, ("tower:fp12_014",), lambda a, b: o.fp12_mul_by_014(a, b[:12], b[12:24], b[24:36])),
    "fp12_frobenius": (12, 0, ("tower:fp12_frob",), lambda a, b: o.fp12_frobenius_map(a)),
    "fp12_conjugate": (12, 0, ("tower:fp12_conj",), lambda a, b: o.fp12_conjugate(a)),
    "fp2_invert": (2, 0, ("inv:fp2",), lambda a, b: _z(12, o.fp2_invert(a[:12]))),
    "fp2_mul_by_nonresidue": (2, 0, ("tower2:fp2_nr",), lambda a, b: _z(12, o.fp2_mul_by_nonresidue(a[:12]))),
    "fp2_mul_fp": (2, 1, ("tower2:fp2_mulfp",), lambda a, b: _z(12, np.concatenate([o.fp_mul(a[:6], b[:6]), o.fp_mul(a[6:12], b[:6])]))),
    "fp6_mul_by_1": (6, 2, ("tower2:fp6_by1",), lambda a, b: _z(36, o.fp6_mul_by_1(a[:36], b[:12]))),
    "fp6_mul_by_01": (6, 4, ("tower2:fp6_by01",), lambda a, b: _z(36, o.fp6_mul_by_01(a[:36], b[:12], b[12:24]))),
    "fp6_mul_by_nonresidue": (6, 0, ("tower2:fp6_nr",), lambda a, b: _z(36, o.fp6_mul_by_nonresidue(a[:36]))),
    "fp6_invert": (6, 0, ("inv:fp6",), lambda a, b: _z(36, o.fp6_invert(a[:36]))),
    "fp12_invert": (12, 0, ("inv:fp12",), lambda a, b: _z(72, o.fp12_invert(a))),
}


def tower_operands(wa, wb, progs):
    """(labels, a records, b records or None): the pool's record shapes, then the searched records of the matching programs"""
    ra = adv.records(wa)
    labels = [nm for nm, _ in ra]
    a = [r for _, r in ra]
    b = None
    if wb:
        rb = adv.records(max(wb, 2))
        b = [rb[(5 * i + 1) % len(rb)][1][:wb] + [0] * (12 - wb) for i in range(len(ra))]
    for v in SEARCHED["vectors"]:
        if v["program"] in progs:
            labels.append(v["label"])
            a.append([H(x) for x in v["a"]][:wa] + [0] * (12 - wa))
            if wb:
                b.append(([H(x) for x in v["b"]] if v.get("b") else a[-1])[:wb] + [0] * (12 - wb))
    while len(a) % 5 == 0 or len(a) % 16 == 0 or len(a) % 7 == 0:      # never a multiple of a kernel's per-wavefront packing
        labels.append("pad:one")
        a.append([1] + [0] * 11)
        if wb:
            b.append([1] + [0] * 11)
    return labels, rec_arr(a), (rec_arr(b) if wb else None)


def run_rotated(fn, a, b, what, labels):
    """fn on (a, b) in pool order and rotated by each offset of ROTATIONS: the same records must come back (the cooperative family
    packs several records into a wavefront; a result must not depend on its neighbours or its lane group)"""
    got = fn(a, b)
    for k in ROTATIONS:
        rot = fn(np.roll(a, k, axis=0), None if b is None else np.roll(b, k, axis=0))
        same(np.roll(rot, -k, axis=0), got, "%s: batch rotated by %d against pool order" % (what, k), lambda i: labels[i])
    return got


@pytest.mark.parametrize("op", sorted(TOWER))
def test_tower_ops_on_adversarial_records(keng, op):
    wa, wb, progs, ref = TOWER[op]
    labels, a, b = tower_operands(wa, wb, progs)
    what = "tower %s family=%s" % (op, keng.family)
    got = run_rotated(lambda x, y: keng.tower_op(op, x, y), a, b, what, labels)
    want = np.stack([ref(a[i], None if b is None else b[i]) for i in range(len(a))])
    same(got, want, what, lambda i: labels[i])


def cyclotomic_records():
    """f^((p^6 - 1)(p^2 + 1)) of adversarial f (in the cyclotomic subgroup, not in Gt) and the identity.  -1 is NOT among them: the
    subgroup has the odd order p^4 - p^2 + 1, so -1 (order 2) lies outside it and outside the contract of the cyclotomic
    operations (Granger-Scott squaring gives 5 for it, the compressed form decompresses to 1).  A record of a proper subfield maps
    to the identity; a few of those stay, the zero record (not invertible) is left out."""
    labels, out = ["identity"], [[1] + [0] * 11]
    recs = [(nm, r) for nm, r in adv.records(12, n_drawn=24) if not nm.startswith(("one-hot", "subfield"))]
    recs = recs[::5] + [(nm, r) for nm, r in adv.records(12, n_drawn=0) if nm.startswith("subfield")][::7]
    recs += [("searched:" + v["label"], [H(x) for x in v["a"]]) for v in SEARCHED["vectors"] if v["program"] in ("ksq", "kdec", "tower:cyc_sqr")]
    for nm, r in recs:
        if not any(r):
            continue
        f = m.f12_from_flat_ints(r)
        t = m.f12_mul(m.f12_conj(f), m.f12_inv(f))
        g = m.f12_mul(m.f12_frob(m.f12_frob(t)), t)
        labels.append("cyc(%s)" % nm)
        out.append(m.f12_flat_ints(g))
    while len(out) % 5 == 0 or len(out) % 16 == 0 or len(out) % 7 == 0:
        labels.append("pad:identity")
        out.append([1] + [0] * 11)
    return labels, rec_arr(out)


def test_cyclotomic_square_and_pow2k(keng):
    """CYCLOTOMIC_SQUARE and CYCLOTOMIC_POW2K at the snapshot bits of |x| and their neighbours"""
    labels, a = cyclotomic_records()
    chain = [a]
    for _ in range(64):
        chain.append(np.stack([o.fp12_cyclotomic_square(r) for r in chain[-1]]))
    what = "tower fp12_cyclotomic_square family=%s" % keng.family
    same(run_rotated(lambda x, y: keng.tower_op("fp12_cyclotomic_square", x), a, None, what, labels), chain[1], what, lambda i: labels[i])
    # -1 lies outside the subgroup (see cyclotomic_records), but the Granger-Scott formulas are polynomial: kernel and oracle must
    # still agree on it bit for bit (3 * 1 - 2 * (-1) = 5 in c0.c0).  Only the squaring: the compressed form of -1 is that of 1.
    minus1 = rec_arr([[P - 1] + [0] * 11, [1] + [0] * 11, [P - 1] + [0] * 11])
    want = np.stack([o.fp12_cyclotomic_square(r) for r in minus1])
    assert o.arr_to_ints(want[0]) == [5] + [0] * 11
    same(keng.tower_op("fp12_cyclotomic_square", minus1), want, what + " on -1", lambda i: ("-1", "identity", "-1")[i])
    for rep in (1, 2, 15, 16, 17, 47, 48, 57, 60, 62, 63, 64):
        what = "tower fp12_cyclotomic_pow2k repeat=%d family=%s" % (rep, keng.family)
        got = run_rotated(lambda x, y: keng.tower_op("fp12_cyclotomic_pow2k", x, None, repeat=rep), a, None, what, labels)
        same(got, chain[rep], what, lambda i: labels[i])


def test_cyclotomic_decompress_all_branches(eng):
    """CYCLOTOMIC_DECOMPRESS (cooperative family) on adversarial (z2 .. z5): the regular branch, z2 == 0 and z2 == z3 == 0, against
    the closed formulas in Python integers; real cyclotomic elements decompress to themselves"""
    clabels, cyc = cyclotomic_records()
    pos = {2: 36, 3: 24, 4: 12, 5: 60}
    labels, recs, want = [], [], []
    for nm, r in adv.records(12, n_drawn=24):
        for branch in (0, 1, 2):
            z = {2: (r[0], r[1]), 3: (r[2], r[3]), 4: (r[4], r[5]), 5: (r[6], r[7])}
            if branch >= 1:
                z[2] = (0, 0)
            if branch == 2:
                z[3] = (0, 0)
            rec = np.zeros(72, dtype=np.uint64)
            rec[0:12] = fp_arr([r[8], r[9]]).reshape(-1)            # whatever sits in z0 and z1 must not matter
            rec[48:60] = fp_arr([r[10], r[11]]).reshape(-1)
            for k, off in pos.items():
                rec[off:off + 12] = fp_arr(z[k]).reshape(-1)
            z0, z1 = _decompress_model(z[2], z[3], z[4], z[5])
            w = rec.copy()
            w[0:12] = fp_arr(z0).reshape(-1)
            w[48:60] = fp_arr(z1).reshape(-1)
            labels.append("%s branch %d" % (nm, branch))
            recs.append(rec)
            want.append(w)
    a = np.concatenate([cyc, np.stack(recs)])
    want = np.concatenate([cyc, np.stack(want)])
    labels = clabels + labels
    if len(a) % 5 == 0 or len(a) % 16 == 0 or len(a) % 7 == 0:
        a, want, labels = a[:-1], want[:-1], labels[:-1]
    what = "tower fp12_cyclotomic_decompress"
    same(run_rotated(lambda x, y: eng.tower_op("fp12_cyclotomic_decompress", x), a, None, what, labels), want, what, lambda i: labels[i])


# ------------------------------------------------------------------------------------------------- final exponentiation
def fexp_operands():
    labels, a, _ = tower_operands(12, 0, ("inv:fp12", "tower:fp12_mul", "tower:fp12_sqr"))
    return labels, a


def fexp_want(a):
    want = o.final_exponentiation_batch(a)
    zero = ~a.any(axis=1)
    want[zero] = 0                                       # final_exponentiation(0) = 0: the zero record (tests/test_coopgen.py)
    return want


def test_final_exponentiation_on_adversarial_records(keng):
    """zkp_final_exponentiation_batch and its _dev flavour on the Fp12 records (zero records among them), in pool order and rotated"""
    import torch
    labels, a = fexp_operands()
    want = fexp_want(a)
    what = "final_exponentiation family=%s" % keng.family
    same(run_rotated(lambda x, y: keng.final_exponentiation(x), a, None, what, labels), want, what, lambda i: labels[i])
    dev = torch.device("cuda", 0)
    got = keng.final_exponentiation(torch.from_numpy(a.view(np.int64)).to(dev)).cpu().numpy().view(np.uint64)
    same(got, want, what + " (_dev)", lambda i: labels[i])


def test_final_exponentiation_shared_inversion_lanes(monkeypatch):
    """the same records with ZKP_COOP_INV_LANES forcing several values per lane of the batched inversion: adversarial norms share a
    Montgomery trick with ordinary ones (and with the zero records, which must not disturb their neighbours)"""
    from zkvm_pairings_amd import PairingEngine
    monkeypatch.setenv("ZKP_COOP_INV_LANES", "16")
    labels, a = fexp_operands()
    g = m.SplitMix64(0xFE)
    rnd = rec_arr([[g.below(P) for _ in range(12)] for _ in range(len(a))])
    mixed = np.empty((2 * len(a), 72), dtype=np.uint64)
    mixed[0::2], mixed[1::2] = a, rnd
    mixed = np.concatenate([mixed, rnd[:3]])             # 2 n + 3: ragged
    lab = lambda i: labels[i // 2] if i % 2 == 0 and i < 2 * len(a) else "random[%d]" % i
    want = fexp_want(mixed)
    e = PairingEngine(0, kernel="coop")
    try:
        what = "final_exponentiation family=coop ZKP_COOP_INV_LANES=16"
        same(run_rotated(lambda x, y: e.final_exponentiation(x), mixed, None, what, [lab(i) for i in range(len(mixed))]), want, what, lab)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------- square roots
def test_fp_sqrt_on_the_pool_and_its_squares(eng):
    ops = adv._dedupe(adv.pool() + searched_fp_ops())
    vals = [op.v for op in ops] + [op.v * op.v % P for op in ops]
    labels = ["%s:%s" % (op.cls, op.name) for op in ops] + ["(%s:%s)^2" % (op.cls, op.name) for op in ops]
    out, sq = eng.fp_sqrt(fp_arr(vals))
    roots = [cm.fp_sqrt(v) for v in vals]
    same(sq, np.array([r is not None for r in roots], dtype=np.uint8), "fp_sqrt is_square", lambda i: labels[i])
    same(out, fp_arr([r or 0 for r in roots]), "fp_sqrt root", lambda i: labels[i])
    assert all(r is not None for r in roots[len(ops):])


def test_fp2_sqrt_on_the_pool_and_its_squares(eng):
    core = adv.core_values()
    vals, labels = [], []
    for k, op in enumerate(core):
        nxt = core[(k + 1) % len(core)]
        for nm, v in (("(v, 0)", (op.v, 0)), ("(0, v)", (0, op.v)), ("(v, v)", (op.v, op.v)), ("(v, next)", (op.v, nxt.v))):
            vals.append(v)
            labels.append("%s %s:%s" % (nm, op.cls, op.name))
            vals.append(m.f2_sqr(v))
            labels.append("%s^2 %s:%s" % (nm, op.cls, op.name))
    a = fp_arr([c for v in vals for c in v]).reshape(-1, 12)
    out, sq = eng.fp2_sqrt(a)
    model = [cm.fp2_sqrt_fast(v) for v in vals]
    same(sq, np.array([r is not None for r in model], dtype=np.uint8), "fp2_sqrt is_square", lambda i: labels[i])
    got = o.arr_to_ints(out)
    for i, v in enumerate(vals):                         # a root it is (Python integers) ...
        r = (got[2 * i], got[2 * i + 1])
        assert (m.f2_sqr(r) == (v[0] % P, v[1] % P)) if model[i] is not None else r == (0, 0), ("fp2_sqrt root", labels[i])
    want = np.stack([_z(12, o.fp2_sqrt(a[i]))[:12] for i in range(len(a))])      # ... and the reference's root, bit for bit
    same(out, want, "fp2_sqrt root against the oracle", lambda i: labels[i])
