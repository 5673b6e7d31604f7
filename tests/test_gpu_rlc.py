"""Batch verification by random linear combination on one MI355X (run with -m gpu): zkp_g1_mul_endo_batch against the oracle's scalar
multiplication, and zkp_pairing_check_batch_rlc on batches whose verdict is known from how they are built - valid checks (free pairs,
Groth16 and BLS shapes, ragged sizes, infinities), bad checks anywhere, two bad checks that cancel in a plain product, invalid points in
every position, zero scalars, host / device / captured-graph flavours and bad arguments.  Expected values come from the oracle
(tests/oracle_lib.py) or from the construction of the inputs - never from the library under test."""
import ctypes
import random

import numpy as np
import pytest

import bls12_381_model as bm
import oracle_lib as o
from replay_cases import free_checks, groth_checks      # the batch builders, shared with the replay and call-order tests

pytestmark = pytest.mark.gpu
P, R = bm.P, bm.R_ORDER
Z2 = bm.BLS_X ** 2
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def _sc(ints):
    return np.stack([o.to_limbs(k % R, 4) for k in ints]) if len(ints) else np.zeros((0, 4), dtype=np.uint64)


def _g1(eng, ks):
    from zkvm_pairings_amd import synthetic
    return eng.g1_mul(synthetic.G1_GENERATOR, _sc(ks))[0]


def _g2(eng, ks):
    from zkvm_pairings_amd import synthetic
    return eng.g2_mul(synthetic.G2_GENERATOR, _sc(ks))[0]


def _ab(rng, n):
    return np.array([[rng.getrandbits(64), rng.getrandbits(64)] for _ in range(n)], dtype=np.uint64).reshape(n, 2)


def _phi(p):
    """(beta x, -y)"""
    x, y = o.from_limbs(p[:6]), o.from_limbs(p[6:])
    return np.concatenate([o.to_limbs(x * bm.BETA % P), o.to_limbs((P - y) % P)])


def _same(got, gi, want, wi):
    if wi:
        ident = np.zeros(12, dtype=np.uint64)
        ident[6] = 1
        return gi == 1 and np.array_equal(got, ident)
    return gi == 0 and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------- the scaling kernel
def test_endo_matches_the_oracle_on_subgroup_points(eng):
    rng = random.Random(0xE0D0)
    n = 300
    base = o.g1_mul_batch(np.tile(o.g1_generator(), (n, 1)), _sc([rng.randrange(1, R) for _ in range(n)]), nthreads=16)
    ab = _ab(rng, n)
    edges = [(0, 0), (1, 0), (0, 1), (M64, 0), (0, M64), (M64, M64), (1, 1), (M64, 1)]
    for i, (a, b) in enumerate(edges):
        ab[i] = (a, b)
    got, gi = eng.g1_mul_endo(base, ab)
    for i in range(n):
        a, b = int(ab[i, 0]), int(ab[i, 1])
        want, wi = o.g1_mul(base[i], (a + b * Z2) % R)
        assert _same(got[i], int(gi[i]), want, wi), i


def test_endo_outside_the_subgroup_and_with_infinities(eng, model_vectors):
    from test_gpu_group import _cofactor_points
    pts = _cofactor_points(model_vectors, 1)
    assert len(pts) >= 4
    rng = random.Random(0xE0D1)
    rows, abs_, inf = [], [], []
    for p in pts:
        for a, b in [(0, 0), (1, 0), (0, 1), (M64, M64), (rng.getrandbits(64), rng.getrandbits(64)), (3, 5)]:
            rows.append(p), abs_.append((a, b)), inf.append(0)
    g = o.g1_generator()
    for a, b in [(7, 9), (0, 0)]:
        rows.append(g), abs_.append((a, b)), inf.append(1)     # a flagged infinity gives the identity whatever its scalars
    base = np.stack(rows)
    ab = np.array(abs_, dtype=np.uint64)
    got, gi = eng.g1_mul_endo(base, ab, np.array(inf, dtype=np.uint8))
    for i, p in enumerate(rows):
        if inf[i]:
            assert _same(got[i], int(gi[i]), None, 1)
            continue
        a, b = abs_[i]
        pa, pai = o.g1_mul(p, a)
        qb, qbi = o.g1_mul(_phi(p), b)
        want, wi = o.g1_add(pa, pai, qb, qbi)
        assert _same(got[i], int(gi[i]), want, wi), (i, a, b)


def test_endo_resident_tensors(eng):
    import torch
    rng = random.Random(0xE0D2)
    n = 130
    base = _g1(eng, [rng.randrange(1, R) for _ in range(n)])
    ab = _ab(rng, n)
    want, wi = eng.g1_mul_endo(base, ab)
    dev = torch.device("cuda", 0)
    tb = torch.from_numpy(base.view(np.int64)).to(dev)
    tab = torch.from_numpy(ab.view(np.int64)).to(dev)
    got, gi = eng.g1_mul_endo(tb, tab)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want) and np.array_equal(gi.cpu().numpy(), wi)


# ------------------------------------------------------------------------------------------------------------------- batch construction
def bls_checks(eng, rng, n, bad=()):
    """e(pk, H) e(-G1, sigma) = 1 with pk = [x]G1, H = [h]G2, sigma = [x h]G2: the generator is the fixed G1 of one column"""
    xv = [rng.randrange(1, R) for _ in range(n)]
    hv = [rng.randrange(1, R) for _ in range(n)]
    sv = [(x * h + (1 if c in bad else 0)) % R for c, (x, h) in enumerate(zip(xv, hv))]
    return dict(g1=_g1(eng, xv), g2=_g2(eng, hv), k=1, col_g2=_g2(eng, sv), fixed_g1=_g1(eng, [R - 1]))


def rlc(eng, g1=None, g2=None, k=0, **kw):
    return eng.pairing_check_rlc(g1, g2, k, **kw)


# ------------------------------------------------------------------------------------------------------------------- valid batches
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_free_only_valid_batches(eng, k):
    rng = random.Random(0xF00 + k)
    g1, g2, i1 = free_checks(eng, rng, 33, k)
    assert rlc(eng, g1, g2, k, inf1=i1) is True


def test_groth16_and_bls_shapes(eng):
    rng = random.Random(0x6016)
    assert rlc(eng, **groth_checks(eng, rng, 100)) is True
    assert rlc(eng, **groth_checks(eng, rng, 40, inf_col=True, inf_fixed=True)) is True
    assert rlc(eng, **bls_checks(eng, rng, 100)) is True
    # columns only (k = 0): the BLS shape with the free pair moved into a fixed-G2 column (e(pk_c, H) with H shared)
    x = [rng.randrange(1, R) for _ in range(20)]
    h = rng.randrange(1, R)
    assert rlc(eng, None, None, 0, col_g1=_g1(eng, x), fixed_g2=_g2(eng, [h]), col_g2=_g2(eng, [xi * h for xi in x]), fixed_g1=_g1(eng, [R - 1])) is True


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1000, 1 << 14])
def test_ragged_batch_sizes(eng, n):
    rng = random.Random(0x5A6 + n)
    g1, g2, i1 = free_checks(eng, rng, n, 2)
    assert rlc(eng, g1, g2, 2, inf1=i1) is True
    if n <= 1000:
        assert rlc(eng, **groth_checks(eng, rng, n, s2=3)) is True


def test_infinities_in_free_column_and_fixed_positions(eng):
    rng = random.Random(0x1AF)
    g1, g2, i1 = free_checks(eng, rng, 50, 3, zero_first=True)
    assert rlc(eng, g1, g2, 3, inf1=i1) is True
    # a flagged G2 infinity in a free pair: that pair drops out, the others must still cancel
    g1, g2, i1 = free_checks(eng, rng, 50, 3, zero_first=True)
    i2 = np.zeros(150, dtype=np.uint8)
    i2[0::3] = 1
    assert rlc(eng, g1, g2, 3, inf1=i1, inf2=i2) is True
    assert rlc(eng, **groth_checks(eng, rng, 64, inf_col=True)) is True
    assert rlc(eng, **groth_checks(eng, rng, 64, inf_fixed=True)) is True


# ------------------------------------------------------------------------------------------------------------------- bad batches
def test_one_bad_check_anywhere(eng):
    rng = random.Random(0xBAD)
    n = 65
    for bad in (0, n // 2, n - 1):
        g1, g2, i1 = free_checks(eng, rng, n, 3, bad={bad})
        assert rlc(eng, g1, g2, 3, inf1=i1) is False
        ok, per = rlc(eng, g1, g2, 3, inf1=i1, locate=True)
        assert ok is False and per.tolist() == [0 if c == bad else 1 for c in range(n)]
        assert rlc(eng, **groth_checks(eng, rng, n, bad={bad})) is False
        assert rlc(eng, **bls_checks(eng, rng, n, bad={bad})) is False


def test_cancelling_bad_checks_pass_the_plain_product_but_not_rlc(eng):
    rng = random.Random(0xCA7)
    t, y = rng.randrange(2, R), rng.randrange(2, R)
    g1 = _g1(eng, [t, R - t])                    # check 0: e([t]G1, [y]G2) != 1; check 1: its inverse
    g2 = _g2(eng, [y, y])
    _, one = eng.pairing_product_check(g1, g2)
    assert one is True
    assert rlc(eng, g1, g2, 1) is False
    ok, per = rlc(eng, g1, g2, 1, locate=True)
    assert per.tolist() == [0, 0]


def test_random_bad_checks_agree_with_pairing_check(eng):
    for seed in range(20):
        rng = random.Random(0x5EED0 + seed)
        n = rng.choice([5, 16, 31, 64])
        bad = {c for c in range(n) if rng.random() < 0.05}
        g1, g2, i1 = free_checks(eng, rng, n, 2, bad=bad)
        kw = groth_checks(eng, rng, n, s2=1, bad={c for c in range(n) if rng.random() < 0.03})
        e1, e2, f1, f2, kk = eng._rlc_expand(n, 1, 0, 1, kw["g1"], kw["g2"], None, None, kw["col_g1"], None, kw["fixed_g2"], None, None, None, None, None)
        per1, all1 = eng.pairing_check(g1, g2, 2, i1)
        per2, all2 = eng.pairing_check(e1, e2, kk, f1, f2)
        assert rlc(eng, g1, g2, 2, inf1=i1, rand=_ab(rng, n)) is all1, seed
        assert rlc(eng, **kw, rand=_ab(rng, n)) is all2, seed


# ------------------------------------------------------------------------------------------------------------------- the points check
def _off_curve(p):
    q = np.array(p, dtype=np.uint64).copy()
    q[6] ^= np.uint64(1)
    return q


def _not_torsion(model_vectors, which):
    for v in model_vectors["groups"]["g1_validity" if which == 1 else "g2_validity"]:
        if v["status"] == 2:
            return o.ints_to_arr([int(h, 16) for h in v["p"]])
    raise AssertionError("no cofactor point in the model vectors")


def test_invalid_points_in_every_position_give_0(eng, model_vectors):
    """each batch holds when its points are taken at face value (the bad point pairs with an infinity or sums with identities), so only
    the points check can reject it: 0 by default, 1 with ZKP_RLC_POINTS_CHECKED"""
    rng = random.Random(0x1A7)
    n = 9
    ident1 = np.tile(o.to_limbs(0, 12), (1, 1)).reshape(12)
    ident1[6] = 1
    ident2 = np.zeros(24, dtype=np.uint64)
    ident2[12] = 1
    for kind in ("off_curve", "not_torsion"):
        bad1 = _off_curve(_g1(eng, [5])[0]) if kind == "off_curve" else _not_torsion(model_vectors, 1)
        bad2 = _off_curve(_g2(eng, [5])[0]) if kind == "off_curve" else _not_torsion(model_vectors, 2)
        base = bls_checks(eng, rng, n)                                      # a valid free pair + fixed-G1 column per check
        ones = np.ones(n, dtype=np.uint8)
        cases = {}
        # free G1: an extra pair (bad1, infinity) per check -> k = 2
        g1 = np.stack([base["g1"], np.tile(bad1, (n, 1))], axis=1).reshape(-1, 12)
        g2 = np.stack([base["g2"], np.tile(ident2, (n, 1))], axis=1).reshape(-1, 24)
        i2 = np.tile([0, 1], n).astype(np.uint8)
        cases["free_g1"] = dict(base, g1=g1, g2=g2, k=2, inf2=i2)
        g1 = np.stack([base["g1"], np.tile(ident1, (n, 1))], axis=1).reshape(-1, 12)
        g2 = np.stack([base["g2"], np.tile(bad2, (n, 1))], axis=1).reshape(-1, 24)
        cases["free_g2"] = dict(base, g1=g1, g2=g2, k=2, inf1=i2.copy())
        # col_g1 bad under an infinite fixed G2; fixed G2 bad under identity columns
        cases["col_g1"] = dict(base, col_g1=np.tile(bad1, (n, 1)), fixed_g2=_g2(eng, [3]), fixed_inf2=np.ones(1, dtype=np.uint8))
        cases["fixed_g2"] = dict(base, col_g1=np.tile(ident1, (n, 1)), col_inf1=ones, fixed_g2=bad2.reshape(1, 24))
        # col_g2 bad under an infinite fixed G1; fixed G1 bad under identity columns (a second fixed-G1 column)
        cases["col_g2"] = dict(base, col_g2=np.concatenate([base["col_g2"][:, None], np.tile(bad2, (n, 1, 1))], axis=1).reshape(-1, 24),
                               fixed_g1=np.concatenate([base["fixed_g1"], _g1(eng, [3])]), fixed_inf1=np.array([0, 1], dtype=np.uint8))
        cases["fixed_g1"] = dict(base, col_g2=np.concatenate([base["col_g2"][:, None], np.tile(ident2, (n, 1, 1))], axis=1).reshape(-1, 24),
                                 col_inf2=np.tile([0, 1], n).astype(np.uint8), fixed_g1=np.concatenate([base["fixed_g1"], bad1[None]]))
        for pos, kw in cases.items():
            assert rlc(eng, **kw) is False, (kind, pos)
            if kind == "not_torsion":
                assert rlc(eng, **kw, points_checked=True) is True, (kind, pos)
            ok, per = rlc(eng, **kw, locate=True)
            assert ok is False and not per.any(), (kind, pos)


def test_a_zero_scalar_gives_0(eng):
    rng = random.Random(0x2E0)
    g1, g2, i1 = free_checks(eng, rng, 10, 2)
    r = _ab(rng, 10)
    assert rlc(eng, g1, g2, 2, inf1=i1, rand=r) is True
    r[4] = (0, 0)
    assert rlc(eng, g1, g2, 2, inf1=i1, rand=r) is False
    r[4] = (0, 1)
    assert rlc(eng, g1, g2, 2, inf1=i1, rand=r) is True


# ------------------------------------------------------------------------------------------------------------------- flavours and arguments
def test_host_dev_and_graph_replay_agree(eng):
    import torch
    dev = torch.device("cuda", 0)
    rng = random.Random(0x6A7)
    t = lambda a: None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    for bad in (set(), {3}):
        kw = groth_checks(eng, rng, 24, bad=bad)
        r = _ab(rng, 24)
        want = rlc(eng, **kw, rand=r)
        assert want is (not bad)
        tkw = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        tr = t(r)
        got = rlc(eng, **tkw, rand=tr)
        torch.cuda.synchronize()
        assert bool(got.item()) is want
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gflag = rlc(eng, **tkw, rand=tr)
        gflag.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert int(gflag.item()) == int(want)


def test_thread_kernel_family(eng):
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0, kernel="thread")
    try:
        rng = random.Random(0x7E)
        assert rlc(e, **groth_checks(e, rng, 12)) is True
        assert rlc(e, **groth_checks(e, rng, 12, bad={5})) is False
        g1, g2, i1 = free_checks(e, rng, 6, 3, bad={0})
        assert rlc(e, g1, g2, 3, inf1=i1) is False
    finally:
        e.close()


def test_empty_batch_and_bad_arguments(eng):
    from zkvm_pairings_amd import _lib
    lib, h = eng._lib, eng._h
    assert rlc(eng, np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64), 1) is True
    one = ctypes.c_int(7)
    b = _lib.RlcBatch(n_checks=0)
    assert lib.zkp_pairing_check_batch_rlc(h, ctypes.byref(b), None, 0, ctypes.byref(one)) == 0 and one.value == 1
    rng = random.Random(0xA76)
    g1, g2, _ = free_checks(eng, rng, 4, 2)
    r = _ab(rng, 4)
    ptr = lambda a: a.ctypes.data

    def call(flags=0, rand=True, all_ok=True, ctx=True, **fields):
        bb = _lib.RlcBatch(n_checks=4, k=2, g1=ptr(g1), g2=ptr(g2))
        for f, v in fields.items():
            setattr(bb, f, v)
        return lib.zkp_pairing_check_batch_rlc(h if ctx else None, ctypes.byref(bb), ptr(r) if rand else None, flags,
                                               ctypes.byref(one) if all_ok else None)

    assert call() == 0
    assert call(ctx=False) == -1
    assert lib.zkp_pairing_check_batch_rlc(h, None, ptr(r), 0, ctypes.byref(one)) == -1
    assert call(rand=False) == -1 and call(all_ok=False) == -1 and call(flags=2) == -1
    assert call(g1=None) == -1 and call(g2=None) == -1
    assert call(k=0) == -1                                             # no pairs at all
    assert call(k=1 << 16) == -1 and call(n_checks=1 << 31, k=1) == -1 and call(n_checks=1 << 20, k=1 << 12) == -1
    assert call(s2=1, fixed_g2=ptr(g2)) == -1                          # a column without its points
    assert call(s1=1, col_g2=ptr(g2)) == -1                            # ... without its fixed point
    assert call(s1=1 << 16, col_g2=ptr(g2), fixed_g1=ptr(g1)) == -1
    assert call(n_checks=(1 << 24) + 1, k=1, s2=1, col_g1=ptr(g1), fixed_g2=ptr(g2)) == -1
    assert lib.zkp_pairing_check_batch_rlc_dev(h, ctypes.byref(_lib.RlcBatch(n_checks=1, k=1)), None, 0, None, None) == -1
    assert lib.zkp_g1_mul_endo_batch(h, None, None, None, 1, None, None) == -1
    assert lib.zkp_g1_mul_endo_batch_dev(None, None, None, None, 0, None, None, None) == -1


def test_validation_mode_covers_every_coordinate_array(eng):
    from zkvm_pairings_amd import PairingEngine, ZkpError
    e = PairingEngine(0, validate=True)
    try:
        rng = random.Random(0x7A1)
        kw = groth_checks(e, rng, 6)
        kw.update(col_g2=_g2(e, [1] * 6), fixed_g1=_g1(e, [1]))
        assert rlc(e, **kw) is False                                   # valid points, an unbalanced column: a plain 0
        for name in ("g1", "g2", "col_g1", "fixed_g2", "col_g2", "fixed_g1"):
            bad = dict(kw)
            a = np.array(bad[name], dtype=np.uint64).copy()
            a.reshape(-1, 6)[-1] = np.uint64(M64)                      # the last Fp of the array >= p
            bad[name] = a
            with pytest.raises(ZkpError) as ei:
                rlc(e, **bad)
            assert ei.value.status == -4, name
    finally:
        e.close()
