"""GPU tests: the pairing entry points on points outside G1 / G2 and off the curves (tests/golden/outside_groups.json), on both kernel
families, against the CPU oracle only.  The entry points do not validate (include/zkp_pairings.h): on any canonical input each returns
exactly final_exponentiation(multi_miller_loop(..)) of the Alg. 26 / 27 formulas, the final exponentiation of zero is zero (so a check
whose Miller value is zero fails), and only the infinity flag marks the identity."""
import numpy as np
import pytest

import bls12_381_model as m
import oracle_lib as o
import outside_groups as og

pytestmark = pytest.mark.gpu

NTHREADS = 16
KS = (1, 2, 3, 8, 9, 16, 17)       # unrolled Miller programs (<= 8), the run-time-k program (9, 16), groups joined by f12mul (17)
GARBAGE1 = (5, 7)                   # canonical coordinates under a set infinity flag
GARBAGE2 = ((1, 2), (3, 4))


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=["thread", "coop"])
def family(request):
    return request.param


@pytest.fixture(scope="module")
def keng(family, eng):
    """the same engine with each Miller/final-exp kernel family selected"""
    from zkvm_pairings_amd import _lib
    try:
        eng.set_kernel(family)
    except _lib.ZkpError:
        pytest.skip("kernel family %s not available in this build" % family)
    yield eng
    eng.set_kernel("auto")


def _special_pairs():
    """(name, P or None, Q or None): every fixture class against the other group's generator, two cross pairs, and flagged
    infinities over garbage (None)"""
    g1, g2 = og.g1_points(), og.g2_points()
    out = [("g1_" + k, p, m.G2_GEN) for k, p in g1.items()] + [("g2_" + k, m.G1_GEN, q) for k, q in g2.items()]
    out += [("zero_c2", g1["off_zero"], g2["off_c2_zero"]), ("order3_order13", g1["order3"], g2["order13"]),
            ("inf1_garbage", None, m.G2_GEN), ("inf2_garbage", m.G1_GEN, None)]
    return out


def _fillers(n, seed):
    """n valid pairs whose pairings multiply to one where n allows it (n = 1 cannot: one pair with e != 1)"""
    rng = m.SplitMix64(seed)
    sc = lambda: 1 + rng.below(m.R_ORDER - 1)
    g1 = lambda a: o.g1_mul(o.g1_generator(), a)[0]
    g2 = lambda b: o.g2_mul(o.g2_generator(), b)[0]
    out = []
    if n % 2 == 1 and n >= 3:
        a, b, q = sc(), sc(), g2(sc())
        out += [(g1(a), q), (g1(b), q), (g1((-(a + b)) % m.R_ORDER), q)]
    elif n % 2 == 1:
        out.append((g1(sc()), g2(sc())))
    while len(out) < n:
        a, q = sc(), g2(sc())
        out += [(g1(a), q), (g1(m.R_ORDER - a), q)]
    return out


_BATCH = {}


def _batch(k):
    """every special pair at every position of a check of k pairs, the rest valid: (g1, g2, inf1, inf2) over n_checks * k pairs, and
    the oracle's Miller values, Gt and ok bytes per check"""
    if k in _BATCH:
        return _BATCH[k]
    fill = _fillers(k - 1, 0xB0B + k)
    g1, g2, i1, i2 = [], [], [], []
    for _, p, q in _special_pairs():
        for pos in range(k):
            row = list(fill)
            row.insert(pos, (og.g1_wire(p if p is not None else GARBAGE1), og.g2_wire(q if q is not None else GARBAGE2)))
            flags1 = [0] * k
            flags2 = [0] * k
            flags1[pos], flags2[pos] = int(p is None), int(q is None)
            g1 += [a for a, _ in row]
            g2 += [b for _, b in row]
            i1 += flags1
            i2 += flags2
    g1, g2 = np.stack(g1), np.stack(g2)
    i1, i2 = np.array(i1, dtype=np.uint8), np.array(i2, dtype=np.uint8)
    nc = g1.shape[0] // k
    ml = o.multi_miller_loop_batch(g1, g2, nc, k, i1, i2)
    gt = o.final_exponentiation_batch(ml)
    ok = np.array([np.array_equal(r, o.fp12_one()) for r in gt], dtype=np.uint8)
    _BATCH[k] = (g1, g2, i1, i2, ml, gt, ok)
    return _BATCH[k]


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def _h(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def test_oracle_batch_has_the_verdicts_it_should():
    """the expectations themselves: zero Miller value -> zero Gt -> failing check; a flagged infinity over garbage contributes one"""
    g1, g2, i1, i2, ml, gt, ok = _batch(3)
    names = [n for n, _, _ in _special_pairs() for _ in range(3)]
    for c, name in enumerate(names):
        if name in ("g2_off_zero", "zero_c2"):
            assert not ml[c].any() and not gt[c].any() and not ok[c], name
        if name.startswith("inf"):
            assert ok[c], name
    one = o.fp12_one()
    assert np.array_equal(o.final_exponentiation_batch(np.stack([one, np.zeros(72, np.uint64)]))[1], np.zeros(72, np.uint64))


@pytest.mark.parametrize("k", KS)
def test_batched_entry_points_on_every_class_and_position(keng, k):
    g1, g2, i1, i2, ml_w, gt_w, ok_w = _batch(k)
    # multi_miller_loop + final_exponentiation, host and device
    ml = keng.multi_miller_loop(g1, g2, k, i1, i2)
    assert np.array_equal(ml, ml_w)
    assert np.array_equal(keng.final_exponentiation(ml), gt_w)
    assert np.array_equal(_h(keng.multi_miller_loop(_t(g1), _t(g2), k, _t(i1), _t(i2))), ml_w)
    assert np.array_equal(_h(keng.final_exponentiation(_t(ml_w))), gt_w)
    # pairing_check: ok bytes and the AND, host and device
    ok, allok = keng.pairing_check(g1, g2, k, i1, i2)
    assert np.array_equal(ok, ok_w) and allok == bool(ok_w.all())
    okd = keng.pairing_check(_t(g1), _t(g2), k, _t(i1), _t(i2))
    assert np.array_equal(_h(okd[0]), ok_w) and bool(_h(okd[1]).reshape(-1)[0]) == bool(ok_w.all())
    # the fused Gt + check pass (zkp_pairing_gt_check_batch_dev): Gt equals final_exponentiation(multi_miller_loop) of the oracle AND of
    # this GPU's own multi_miller_loop, byte for byte
    import torch
    nc = ml_w.shape[0]
    out = torch.empty((nc, 72), dtype=torch.int64, device="cuda:0")
    okt = torch.empty(nc, dtype=torch.uint8, device="cuda:0")
    allt = torch.ones(1, dtype=torch.int32, device="cuda:0")
    keng.pairing_gt_check(_t(g1), _t(g2), k, out, okt, allt, _t(i1), _t(i2))
    gt = _h(out)
    assert np.array_equal(gt, gt_w) and np.array_equal(gt, keng.final_exponentiation(ml))
    assert np.array_equal(_h(okt), ok_w) and bool(_h(allt)[0]) == bool(ok_w.all())


@pytest.mark.parametrize("k", (1, 3, 17))
def test_pairing_equals_final_exponentiation_of_the_miller_loop(keng, k):
    """pairing() of every pair of the batch (each pair its own pairing, flagged infinities included), host and device, against the
    oracle and against this GPU's own final_exponentiation(multi_miller_loop) row by row"""
    g1, g2, i1, i2, _, _, _ = _batch(k)
    want = o.pairing_batch(g1, g2, i1, i2, NTHREADS)
    got = keng.pairing(g1, g2, i1, i2)
    assert np.array_equal(got, want)
    assert np.array_equal(got, keng.final_exponentiation(keng.multi_miller_loop(g1, g2, 1, i1, i2)))
    assert np.array_equal(_h(keng.pairing(_t(g1), _t(g2), _t(i1), _t(i2))), want)


@pytest.mark.parametrize("k", (1, 2, 9, 17))
def test_one_product_check_entry_points(keng, k):
    """zkp_miller_product / zkp_pairing_product_check (host and device) on each check of the batch at its first, middle and last
    position: the Miller value, Gt and is_one of the oracle"""
    g1, g2, i1, i2, ml_w, gt_w, ok_w = _batch(k)
    for c in range(ml_w.shape[0]):
        if c % k not in (0, k // 2, k - 1):
            continue
        s = slice(c * k, (c + 1) * k)
        a1, a2, f1, f2 = g1[s], g2[s], i1[s], i2[s]
        assert np.array_equal(keng.miller_product(a1, a2, f1, f2), ml_w[c]), c
        gt, one = keng.pairing_product_check(a1, a2, f1, f2)
        assert np.array_equal(gt, gt_w[c]) and one == bool(ok_w[c]), c
        assert np.array_equal(_h(keng.miller_product(_t(a1), _t(a2), _t(f1), _t(f2))), ml_w[c]), c
        gtd, oned = keng.pairing_product_check(_t(a1), _t(a2), _t(f1), _t(f2))
        assert np.array_equal(_h(gtd), gt_w[c]) and bool(_h(oned)[0]) == bool(ok_w[c]), c


@pytest.mark.parametrize("k", (1, 3, 9))
def test_two_context_calls(keng, family, k):
    """zkp_pairing_batch_multi / zkp_pairing_check_batch_multi over two contexts of the same family"""
    from zkvm_pairings_amd import PairingEngine, multi
    g1, g2, i1, i2, _, gt_w, ok_w = _batch(k)
    other = PairingEngine(0)
    try:
        other.set_kernel(family)
        ok, allok = multi.pairing_check_multi([keng, other], g1, g2, k, i1, i2)
        assert np.array_equal(ok, ok_w) and allok == bool(ok_w.all())
        if k == 1:
            gt, ok1, all1 = multi.pairing_multi([keng, other], g1, g2, i1, i2)
            assert np.array_equal(gt, gt_w) and np.array_equal(ok1, ok_w) and all1 == bool(ok_w.all())
    finally:
        other.close()


def _fexp_rows(n, zeros, seed):
    """n Miller values of valid random pairs with the rows in `zeros` set to zero, and the oracle's final exponentiation"""
    g = m.SplitMix64(seed)
    a = np.stack([o.g1_mul(o.g1_generator(), 1 + g.below(m.R_ORDER - 1))[0] for _ in range(8)])
    b = np.stack([o.g2_mul(o.g2_generator(), 1 + g.below(m.R_ORDER - 1))[0] for _ in range(8)])
    base = o.multi_miller_loop_batch(a, b, 8, 1)
    f = np.stack([base[i % 8] for i in range(n)])
    for z in zeros:
        f[z] = 0
    want = o.final_exponentiation_batch(f)
    for z in zeros:
        assert not want[z].any()
    return f, want


def test_final_exponentiation_of_zero_rows(keng):
    """zero rows first, in the middle and last: zero out, and the batched (Montgomery) inversion of the other rows is not spoiled"""
    for n, zeros in ((1, (0,)), (3, (1,)), (40, (0, 17, 39)), (70, (0, 1, 2, 35, 69))):
        f, want = _fexp_rows(n, zeros, n)
        assert np.array_equal(keng.final_exponentiation(f), want), n
        assert np.array_equal(_h(keng.final_exponentiation(_t(f))), want), n


def test_final_exponentiation_of_zero_rows_across_chunks(monkeypatch, family):
    """the same with the cooperative pipeline forced to chunks of 320 checks over three streams and two super-chunks: zeros at and
    around the chunk boundaries"""
    from zkvm_pairings_amd import PairingEngine
    monkeypatch.setenv("ZKP_COOP_CHUNK", "320")
    monkeypatch.setenv("ZKP_COOP_STREAMS", "3")
    monkeypatch.setenv("ZKP_COOP_SUPER", "640")
    e = PairingEngine(0)
    try:
        e.set_kernel(family)
        zeros = (0, 319, 320, 321, 639, 640, 700)
        f, want = _fexp_rows(701, zeros, 7)
        assert np.array_equal(e.final_exponentiation(f), want)
        assert np.array_equal(_h(e.final_exponentiation(_t(f))), want)
        # and every special pair, repeated over 701 one-pair checks: the classes cross the chunk and super-chunk edges
        g1, g2, i1, i2, _, _, _ = _batch(1)
        idx = np.arange(701) % g1.shape[0]
        g1, g2, i1, i2 = g1[idx], g2[idx], i1[idx], i2[idx]
        gt_w = o.pairing_batch(g1, g2, i1, i2, NTHREADS)
        ok_w = np.array([np.array_equal(r, o.fp12_one()) for r in gt_w], dtype=np.uint8)
        ok, allok = e.pairing_check(g1, g2, 1, i1, i2)
        assert np.array_equal(ok, ok_w) and not allok
        assert np.array_equal(e.pairing(g1, g2, i1, i2), gt_w)
        assert np.array_equal(e.multi_miller_loop(g1, g2, 1, i1, i2), o.multi_miller_loop_batch(g1, g2, 701, 1, i1, i2))
    finally:
        e.close()
