"""Group addition and multi-scalar multiplication on one MI355X (run with -m gpu): zkp_g*_add_batch against the oracle's affine Add
(random pairs, every exceptional case, points outside the subgroup), zkp_g*_msm_batch against the oracle's sum of multiples and, at
scale, against a construction (bases [a_i]G, so that sum k_i [a_i]G = [sum k_i a_i mod r]G needs one oracle multiplication), the
resident-tensor path and a captured, replayed MSM.  Expected values come from the oracle (tests/oracle_lib.py) or from the
construction of the inputs - never from the library under test."""
import random

import numpy as np
import pytest

import bls12_381_model as bm
import oracle_lib as o

pytestmark = pytest.mark.gpu
P, R = bm.P, bm.R_ORDER
EDGE = [0, 1, R - 1, R, 1 << 255, (1 << 256) - 1]
COLS = {1: 12, 2: 24}


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def _gen(which):
    return o.g1_generator() if which == 1 else o.g2_generator()


def _sc(ints):
    return np.stack([o.to_limbs(k, 4) for k in ints]) if ints else np.zeros((0, 4), dtype=np.uint64)


def _neg(which, p):
    q = np.array(p, dtype=np.uint64).copy()
    ys = [slice(6, 12)] if which == 1 else [slice(12, 18), slice(18, 24)]
    for s in ys:
        q[s] = o.to_limbs((P - o.from_limbs(q[s])) % P)
    return q


def _omul(which, p, k, inf=0):
    return (o.g1_mul if which == 1 else o.g2_mul)(p, k, inf)


def _oadd(which, p, pi, q, qi):
    return (o.g1_add if which == 1 else o.g2_add)(p, pi, q, qi)


def _points(eng, which, ks):
    """[k]G for the given ints, computed by the oracle"""
    return np.stack([_omul(which, _gen(which), k)[0] for k in ks])


def _assert_same(which, got, gi, want, wi):
    """an infinite result is (0, 1) with the flag set; a finite one equals the oracle's bit for bit"""
    if wi:
        ident = np.zeros(COLS[which], dtype=np.uint64)
        ident[6 * which] = 1
        assert gi == 1 and np.array_equal(got, ident)
    else:
        assert gi == 0 and np.array_equal(got, want)


def _oracle_msm(which, pts, inf, ks):
    acc, ai = np.zeros(COLS[which], dtype=np.uint64), 1
    for p, i, k in zip(pts, inf, ks):
        q, qi = _omul(which, p, k, int(i))
        acc, ai = _oadd(which, acc, ai, q, qi)
    return acc, ai


# ------------------------------------------------------------------------------------------------------------------- addition
@pytest.mark.parametrize("which", [1, 2])
def test_add_random_pairs_match_the_oracle(eng, which):
    rng = np.random.default_rng(0xADD + which)
    n = 4096
    ka = [int(x) for x in rng.integers(1, 1 << 62, n)]
    kb = [int(x) for x in rng.integers(1, 1 << 62, n)]
    base = np.tile(_gen(which), (n, 1))
    mulb = o.g1_mul_batch if which == 1 else o.g2_mul_batch
    a, b = mulb(base, _sc(ka), nthreads=16), mulb(base, _sc(kb), nthreads=16)
    got, gi = (eng.g1_add if which == 1 else eng.g2_add)(a, b)
    for i in range(n):
        w, wi = _oadd(which, a[i], 0, b[i], 0)
        _assert_same(which, got[i], int(gi[i]), w, wi)


@pytest.mark.parametrize("which", [1, 2])
def test_add_exceptional_cases(eng, which):
    p = _points(eng, which, [0x1234567])[0]
    q = _points(eng, which, [0x7654321])[0]
    np_ = _neg(which, p)
    cases = [(p, 0, p, 0), (p, 0, np_, 0), (p, 0, q, 1), (q, 1, p, 0), (p, 1, q, 1), (np_, 0, p, 0), (p, 0, q, 0)]
    a = np.stack([c[0] for c in cases])
    b = np.stack([c[2] for c in cases])
    ia = np.array([c[1] for c in cases], dtype=np.uint8)
    ib = np.array([c[3] for c in cases], dtype=np.uint8)
    got, gi = (eng.g1_add if which == 1 else eng.g2_add)(a, b, ia, ib)
    for i, (x, xi, y, yi) in enumerate(cases):
        w, wi = _oadd(which, x, xi, y, yi)
        _assert_same(which, got[i], int(gi[i]), w, wi)
    assert gi.tolist() == [0, 1, 0, 0, 1, 1, 0]            # P + (-P) and inf + inf are the identity


def _cofactor_points(model_vectors, which):
    pts = []
    for v in model_vectors["groups"]["g1_validity" if which == 1 else "g2_validity"]:
        if v["status"] == 2:
            base = o.ints_to_arr([int(h, 16) for h in v["p"]])
            tors, inf = _omul(which, base, R)                # order divides the cofactor
            if not inf:
                pts.append(tors)
                pts.append(base)
    if which == 1:
        pts += [o.ints_to_arr([0, 2]), o.ints_to_arr([0, P - 2])]
    return pts


@pytest.mark.parametrize("which", [1, 2])
def test_add_points_outside_the_subgroup(eng, model_vectors, which):
    pts = _cofactor_points(model_vectors, which)
    assert len(pts) >= 4
    pairs = [(x, y) for x in pts for y in pts] + [(x, _neg(which, x)) for x in pts]
    a, b = np.stack([x for x, _ in pairs]), np.stack([y for _, y in pairs])
    got, gi = (eng.g1_add if which == 1 else eng.g2_add)(a, b)
    for i, (x, y) in enumerate(pairs):
        w, wi = _oadd(which, x, 0, y, 0)
        _assert_same(which, got[i], int(gi[i]), w, wi)


# ------------------------------------------------------------------------------------------------------------------- MSM vs oracle
@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("m,n_msm", [(1, 1), (2, 5), (3, 1), (7, 5), (64, 1), (64, 5), (1000, 1), (1, 300), (3, 300)])
@pytest.mark.parametrize("shared", [False, True])
def test_msm_matches_the_oracle(eng, which, m, n_msm, shared):
    if which == 2 and m * n_msm > 1000:
        pytest.skip("G2 at this size: covered by the construction tests")
    rng = random.Random(m * 1000003 + n_msm * 7 + shared + 10 * which)
    n_pts = m if shared else m * n_msm
    pts = _points(eng, which, [rng.randrange(1, R) for _ in range(min(n_pts, 64))])
    pts = pts[[rng.randrange(len(pts)) for _ in range(n_pts)]]          # duplicates on purpose
    ks = [rng.choice(EDGE) if rng.random() < 0.2 else rng.getrandbits(256) for _ in range(m * n_msm)]
    got, gi = (eng.g1_msm if which == 1 else eng.g2_msm)(pts, _sc(ks), n_msm, None, shared)
    inf = np.zeros(n_pts, dtype=np.uint8)
    for j in range(n_msm):
        sp = pts if shared else pts[j * m:(j + 1) * m]
        w, wi = _oracle_msm(which, sp, inf[:m], ks[j * m:(j + 1) * m])
        _assert_same(which, got[j], int(gi[j]), w, wi)


@pytest.mark.parametrize("which", [1, 2])
def test_msm_edge_scalars_duplicates_cancellation_and_infinity(eng, which):
    p, q = _points(eng, which, [0xBEEF, 0xF00D])
    segs = [
        ([p] * 6, [0] * 6, EDGE),                                          # every edge scalar
        ([p] * 6, [0] * 6, [0] * 6),                                       # all zero scalars
        ([p, _neg(which, p)], [0, 0], [5, 5]),                             # P next to -P: cancels to infinity
        ([p, q, p, q], [0, 1, 0, 1], [3, 9, 4, 1]),                        # infinity inputs (their scalars ignored)
        ([p, q, p], [1, 1, 1], [1, 2, 3]),                                 # all-infinity segment
        ([p, q, _neg(which, q)], [0, 0, 0], [R - 1, 7, 7]),                # r - 1 and a cancelling pair
    ]
    m = 6
    pts, infs, ks = [], [], []
    for sp, si, sk in segs:                                                # pad to m terms with zero scalars
        pts += sp + [q] * (m - len(sp))
        infs += si + [0] * (m - len(si))
        ks += list(sk) + [0] * (m - len(sk))
    pts, infs = np.stack(pts), np.array(infs, dtype=np.uint8)
    got, gi = (eng.g1_msm if which == 1 else eng.g2_msm)(pts, _sc(ks), len(segs), infs)
    for j in range(len(segs)):
        w, wi = _oracle_msm(which, pts[j * m:(j + 1) * m], infs[j * m:(j + 1) * m], ks[j * m:(j + 1) * m])
        _assert_same(which, got[j], int(gi[j]), w, wi)
    assert gi.tolist() == [0, 1, 1, 0, 1, 0]


# ------------------------------------------------------------------------------------------------------------------- MSM by construction
def _constructed(eng, which, m, seed, equal=False):
    """bases [a_i]G (a_i small, computed on the device by the scalar multiplication: they are inputs) and scalars; expected by one
    oracle multiplication"""
    rng = np.random.default_rng(seed)
    a = [int(x) for x in rng.integers(1, 1 << 40, m)]
    base, _ = (eng.g1_mul if which == 1 else eng.g2_mul)(_gen(which), _sc(a))
    if equal:
        ks = [int.from_bytes(rng.bytes(32), "little")] * m
    else:
        ks = [int.from_bytes(rng.bytes(32), "little") for _ in range(m)]
    return base, a, ks


def _expect(which, a, ks):
    s = sum(k * x for k, x in zip(ks, a)) % R
    return _omul(which, _gen(which), s)


@pytest.mark.parametrize("which,log_m", [(1, 20), (2, 18)])
def test_msm_at_scale_by_construction(eng, which, log_m):
    base, a, ks = _constructed(eng, which, 1 << log_m, 0x5CA1E + which)
    got, gi = (eng.g1_msm if which == 1 else eng.g2_msm)(base, _sc(ks))
    w, wi = _expect(which, a, ks)
    _assert_same(which, got[0], int(gi[0]), w, wi)


@pytest.mark.parametrize("which", [1, 2])
def test_msm_all_scalars_equal_one_bucket(eng, which):
    base, a, ks = _constructed(eng, which, 1 << 14, 0xB0C + which, equal=True)
    got, gi = (eng.g1_msm if which == 1 else eng.g2_msm)(base, _sc(ks))
    w, wi = _expect(which, a, ks)
    _assert_same(which, got[0], int(gi[0]), w, wi)


def test_msm_many_small_sums_shared_bases(eng):
    m, n_msm = 64, 1 << 14
    base, a, _ = _constructed(eng, 1, m, 0x64)
    rng = np.random.default_rng(0x6464)
    sc = rng.integers(0, 1 << 63, (m * n_msm, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (m * n_msm, 4), dtype=np.uint64)
    got, gi = eng.g1_msm(base, sc, n_msm, None, True)
    for j in list(range(0, n_msm, 1021)) + [n_msm - 1]:
        ks = [o.from_limbs(sc[j * m + i]) for i in range(m)]
        w, wi = _expect(1, a, ks)
        _assert_same(1, got[j], int(gi[j]), w, wi)


# ------------------------------------------------------------------------------------------------------------------- resident path
@pytest.mark.parametrize("which", [1, 2])
def test_dev_path_and_graph_replay_give_the_same_bytes(eng, which):
    import torch
    dev = torch.device("cuda", 0)
    m, n_msm = 700, 3
    base, _, ks = _constructed(eng, which, m * n_msm, 0xD0 + which)
    sc = _sc(ks)
    want, wi = (eng.g1_msm if which == 1 else eng.g2_msm)(base, sc, n_msm)
    tb = torch.from_numpy(base.view(np.int64)).to(dev)
    ts = torch.from_numpy(sc.view(np.int64)).to(dev)
    fn = eng.g1_msm if which == 1 else eng.g2_msm
    out, oi = fn(tb, ts, n_msm)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want) and np.array_equal(oi.cpu().numpy(), wi)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gout, goi = fn(tb, ts, n_msm)
    gout.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(gout.cpu().numpy().view(np.uint64), want) and np.array_equal(goi.cpu().numpy(), wi)
    # addition through the resident path
    a, b = tb[:16], tb[16:32]
    s, si = (eng.g1_add if which == 1 else eng.g2_add)(a, b)
    hs, hsi = (eng.g1_add if which == 1 else eng.g2_add)(base[:16], base[16:32])
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy().view(np.uint64), hs) and np.array_equal(si.cpu().numpy(), hsi)


def test_python_api(eng):
    from zkvm_pairings_amd import G1Affine, G2Affine, msm
    g, h = G1Affine.generator(), G2Affine.generator()
    w2, _ = _omul(1, _gen(1), 2)
    assert g.double() == G1Affine.from_array(w2) and (g + g) == G1Affine.from_array(w2)
    assert (g - g).is_identity() and (h - h).is_identity() and not (h + h).is_identity()
    ni = -G1Affine.identity()
    assert ni.is_infinity and ni.y == P - 1 and ni.x == 0
    w5, _ = _omul(1, _gen(1), 5)
    assert msm([g, g, G1Affine.identity()], [2, 3, 9]) == G1Affine.from_array(w5)
    w7, _ = _omul(2, _gen(2), 7)
    assert msm([h, -h], [10, 3]) == G2Affine.from_array(w7)


def test_bad_arguments(eng):
    from zkvm_pairings_amd import ZkpError
    g = _gen(1)[None, :]
    with pytest.raises(ValueError):
        eng.g1_msm(np.tile(g, (3, 1)), _sc([1, 2]), 1)
    for m, n_msm in (((1 << 12) + 1, 1 << 12), (0, 1), ((1 << 24) + 1, 1)):    # m * n_msm above 2^24, m = 0: ZKP_ERR_ARG before any access
        assert eng._lib.zkp_g1_msm_batch(eng._h, None, None, None, m, n_msm, 1, None, None) == -1
    bad = g.copy()
    bad[0, :6] = o.to_limbs(P)
    from zkvm_pairings_amd import PairingEngine
    v = PairingEngine(0, validate=True)
    try:
        with pytest.raises(ZkpError) as ei:
            v.g1_add(bad, g)
        assert ei.value.status == -4                                       # ZKP_ERR_NONCANONICAL
        with pytest.raises(ZkpError):
            v.g1_msm(bad, _sc([3]))
    finally:
        v.close()
