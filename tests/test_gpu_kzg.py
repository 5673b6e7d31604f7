"""The batch KZG opening verifier on one MI355X (run with -m gpu): batches from synthetic.kzg_instance, whose verdict is known from how they
are built (secret exponents) - valid batches, one bad opening anywhere (commitment, proof, value, point), non-canonical values, two bad
openings that cancel in a plain sum, zero scalars, the zero polynomial, points outside the groups in every position, host / device /
captured-graph flavours, bad arguments - the per-opening path kzg_verify_each, which is composed of calls that do not know KZG, and the
blob path (evaluation form in, verdict out)."""
import ctypes
import random

import numpy as np
import pytest

import outside_groups as og

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
NS = [1, 2, 5, 127, 1000]


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


_cache = {}


def instance(eng, n):
    """(setup, C, z, y, proofs) of a valid batch; cached, callers copy what they change"""
    from zkvm_pairings_amd import KzgSetup, synthetic
    if n not in _cache:
        setup, c, z, y, p = synthetic.kzg_instance(0x7A6000 + n, n, engine=eng)
        _cache[n] = (KzgSetup(*setup), c, z, y, p)
    return _cache[n]


def rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def to_int(row):
    return int.from_bytes(np.ascontiguousarray(row).tobytes(), "little")


def g1_times(eng, k):
    from zkvm_pairings_amd import synthetic
    return eng.g1_mul(synthetic.G1_GENERATOR, rows([k % R]))[0][0]


def shifted(eng, pts, idx, k=1):
    """pts with pts[idx] + [k] G1"""
    pts = pts.copy()
    for i in idx:
        s, inf = eng.g1_add(pts[i], g1_times(eng, k))
        assert not inf[0]
        pts[i] = s[0]
    return pts


def verify(eng, setup, c, z, y, p, **kw):
    from zkvm_pairings_amd import kzg_verify_batch
    return kzg_verify_batch(setup, c, z, y, p, engine=eng, **kw)


@pytest.mark.parametrize("n", NS)
def test_valid_batches_pass_and_one_bad_opening_fails(eng, n):
    setup, c, z, y, p = instance(eng, n)
    assert verify(eng, setup, c, z, y, p) is True
    assert verify(eng, setup, c, z, y, p, points_checked=True, vk_checked=True) is True
    for idx in sorted({0, n // 2, n - 1}):                  # first, middle, last
        assert verify(eng, setup, shifted(eng, c, [idx]), z, y, p) is False, (idx, "C")
        assert verify(eng, setup, c, z, y, shifted(eng, p, [idx])) is False, (idx, "pi")
        for which in (0, 1):                                # a changed z, a changed y; then z + r, y + r: the same residue, not the same input
            v = to_int((z, y)[which][idx])
            zy = [z.copy(), y.copy()]
            zy[which][idx] = rows([(v + 1) % R])[0]
            assert verify(eng, setup, c, zy[0], zy[1], p) is False, (idx, which)
            assert v + R < 1 << 256
            zy[which][idx] = rows([v + R])[0]
            assert verify(eng, setup, c, zy[0], zy[1], p) is False, (idx, which, "+ r")
            assert verify(eng, setup, c, zy[0], zy[1], p, points_checked=True, vk_checked=True) is False


def test_synthetic_bad_list_marks_exactly_those_openings(eng):
    from zkvm_pairings_amd import KzgSetup, kzg_verify_each, synthetic
    n = 9
    setup, c, z, y, p = synthetic.kzg_instance(0xBAD, n, bad=(0, 4, 8), engine=eng)
    setup = KzgSetup(*setup)
    assert verify(eng, setup, c, z, y, p) is False
    assert kzg_verify_each(setup, c, z, y, p, engine=eng).tolist() == [i not in (0, 4, 8) for i in range(n)]
    setup2, c2, z2, y2, p2 = synthetic.kzg_instance(0xBAD, n, engine=eng)
    assert np.array_equal(c2, shifted(eng, c, [0, 4, 8], k=R - 1)) and np.array_equal(z, z2) and np.array_equal(y, y2) and np.array_equal(p, p2)
    assert verify(eng, KzgSetup(*setup2), c2, z2, y2, p2) is True


@pytest.mark.parametrize("n", [2, 5, 127, 1000])
def test_two_bad_openings_that_cancel_in_a_plain_sum_fail(eng, n):
    setup, c, z, y, p = instance(eng, n)
    i, j = 0, n - 1
    bad = shifted(eng, shifted(eng, c, [i], k=17), [j], k=R - 17)     # C_i + D, C_j - D: the plain sum of the commitments is unchanged
    assert verify(eng, setup, bad, z, y, p) is False
    # with equal scalars on the two openings the combination cannot tell - this is why the scalars are random
    rand = eng.rlc_random(n)
    rand[j] = rand[i]
    assert verify(eng, setup, bad, z, y, p, rand=rand) is True


def test_zero_scalars_fail(eng):
    for n in (1, 5, 127):
        setup, c, z, y, p = instance(eng, n)
        for idx in sorted({0, n // 2, n - 1}):
            rand = eng.rlc_random(n)
            rand[idx] = 0
            assert verify(eng, setup, c, z, y, p, rand=rand) is False
            assert verify(eng, setup, c, z, y, p, rand=rand, points_checked=True, vk_checked=True) is False
        rand = eng.rlc_random(n)
        rand[:, 1] = 0                                        # (a, 0) and (0, b) are legal scalars
        assert verify(eng, setup, c, z, y, p, rand=rand) is True
        rand = eng.rlc_random(n)
        rand[:, 0] = 0
        assert verify(eng, setup, c, z, y, p, rand=rand) is True


def test_the_zero_polynomial_opens_with_infinities(eng):
    from zkvm_pairings_amd import kzg_verify_each
    n = 5
    setup, c, z, y, p = instance(eng, n)
    for idx in ([2], [0, 4], list(range(n))):
        ic, ip, yy = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), y.copy()
        for i in idx:
            ic[i] = ip[i] = 1                                 # C = infinity, pi = infinity, y = 0, any z
            yy[i] = 0
        assert verify(eng, setup, c, z, yy, p, inf_c=ic, inf_proof=ip) is True, idx
        assert kzg_verify_each(setup, c, z, yy, p, engine=eng, inf_c=ic, inf_proof=ip).all()
        assert verify(eng, setup, c, z, y, p, inf_c=ic, inf_proof=ip) is False, idx      # ... but not to y != 0
    ic = np.zeros(n, dtype=np.uint8)
    ic[1] = 1
    assert verify(eng, setup, c, z, y, p, inf_c=ic) is False      # a flagged infinity is a valid point, the opening is false


def test_points_outside_the_groups_fail_in_every_position(eng):
    from zkvm_pairings_amd import KzgSetup
    n = 2
    setup, c, z, y, p = instance(eng, n)
    g1s = {k: og.g1_wire(pt) for k, pt in og.g1_points().items()}
    g2s = {k: og.g2_wire(q) for k, q in og.g2_points().items()}
    assert len(g1s) >= 2 and len(g2s) >= 2
    for name, pt in g1s.items():
        for pos in range(n):
            for which in (0, 1):
                cp = [c.copy(), p.copy()]
                cp[which][pos] = pt
                assert verify(eng, setup, cp[0], z, y, cp[1]) is False, (name, pos, which)
        assert verify(eng, KzgSetup(pt, setup.g2, setup.tau_g2), c, z, y, p) is False, name
    for name, q in g2s.items():
        assert verify(eng, KzgSetup(setup.g1, q, setup.tau_g2), c, z, y, p) is False, (name, "g2")
        assert verify(eng, KzgSetup(setup.g1, setup.g2, q), c, z, y, p) is False, (name, "tau_g2")


def test_empty_batch_passes(eng):
    from zkvm_pairings_amd import _lib
    setup, _, _, _, _ = instance(eng, 1)
    e = np.zeros((0, 12), dtype=np.uint64)
    assert verify(eng, setup, e, np.zeros((0, 4)), np.zeros((0, 4)), e) is True
    res = ctypes.c_int(5)
    kv, bt = _lib.KzgVk(), _lib.KzgBatch(n=0)
    assert eng._lib.zkp_kzg_verify_batch(eng._h, ctypes.byref(kv), ctypes.byref(bt), None, 0, ctypes.byref(res)) == 0 and res.value == 1
    import torch
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
    assert eng._lib.zkp_kzg_verify_batch_dev(eng._h, ctypes.byref(kv), ctypes.byref(bt), None, 0, ctypes.c_void_p(flag.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 1


@pytest.mark.parametrize("n,seed", [(5, 1), (127, 2), (1000, 3)])
def test_batch_verdict_equals_all_of_verify_each_on_mixed_batches(eng, n, seed):
    from zkvm_pairings_amd import kzg_verify_each
    rng = random.Random(0xEAC1 + seed)
    setup, c, z, y, p = instance(eng, n)
    assert kzg_verify_each(setup, c, z, y, p, engine=eng).all() and verify(eng, setup, c, z, y, p) is True
    for trial in range(3):
        bad_c = sorted(rng.sample(range(n), rng.choice([0, 1, 2])))
        bad_p = sorted(rng.sample(range(n), rng.choice([0, 1])))
        bad_y = sorted(rng.sample(range(n), rng.choice([0, 1])))
        non_canonical = sorted(rng.sample(range(n), rng.choice([0, 1])))
        cc, pp, yy, zz = shifted(eng, c, bad_c, k=rng.randrange(1, R)), shifted(eng, p, bad_p, k=rng.randrange(1, R)), y.copy(), z.copy()
        for i in bad_y:
            yy[i] = rows([(to_int(yy[i]) + rng.randrange(1, R)) % R])[0]
        for i in non_canonical:
            zz[i] = rows([to_int(zz[i]) + R])[0]
        want = [i not in bad_c and i not in bad_p and i not in bad_y and i not in non_canonical for i in range(n)]     # by construction
        assert kzg_verify_each(setup, cc, zz, yy, pp, engine=eng).tolist() == want, trial
        assert verify(eng, setup, cc, zz, yy, pp) is all(want), trial


def tensors(arrs):
    import torch
    d = torch.device("cuda", 0)
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(d) for a in arrs]


@pytest.mark.parametrize("n", [1, 5, 127])
def test_host_dev_and_graph_replay_agree(eng, n):
    import torch
    setup, c, z, y, p = instance(eng, n)
    for cc, want in ((c, True), (shifted(eng, c, [n // 2]), False)):
        rand = eng.rlc_random(n)
        assert eng.kzg_verify_batch(*setup.arrays(), cc, z, y, p, rand=rand) is want
        tk = tensors(setup.arrays())
        tc, tz, ty, tp = tensors([cc, z, y, p])
        tr = torch.from_numpy(rand.view(np.int64)).to(tz.device)
        got = eng.kzg_verify_batch(*tk, tc, tz, ty, tp, rand=tr)
        torch.cuda.synchronize()
        assert got.dtype == torch.int32 and bool(got.item()) is want
        for kw in ({}, {"points_checked": True, "vk_checked": True}):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gflag = eng.kzg_verify_batch(*tk, tc, tz, ty, tp, rand=tr, **kw)
            for _ in range(2):
                gflag.fill_(7)
                graph.replay()
                torch.cuda.synchronize()
                assert int(gflag.item()) == int(want)


def test_the_largest_batch_forms_its_sums_by_two_msm_calls(eng):
    """n = 2^22, the ABI's limit: two rows of 2 n + 1 terms exceed the MSM's 2^24, so this size alone takes the two-call path (every other
    test runs the one shared-bases call).  A valid batch of 1024 openings tiled on the device; then the last opening made false."""
    import torch
    n, nb = 1 << 22, 1024
    setup, c, z, y, p = instance(eng, nb)
    tk = tensors(setup.arrays())
    tc, tz, ty, tp = (t.repeat(n // nb, 1) for t in tensors([c, z, y, p]))
    (tr,) = tensors([eng.rlc_random(n)])
    assert int(eng.kzg_verify_batch(*tk, tc, tz, ty, tp, rand=tr).item()) == 1
    tc[n - 1] = tensors([shifted(eng, c, [nb - 1])])[0][nb - 1]
    assert int(eng.kzg_verify_batch(*tk, tc, tz, ty, tp, rand=tr).item()) == 0


def test_validation_mode_keeps_the_rule_for_coordinates_and_not_for_scalars(eng):
    from zkvm_pairings_amd import KzgSetup, PairingEngine, ZkpError
    e = PairingEngine(0, validate=True)
    try:
        n = 2
        setup, c, z, y, p = instance(eng, n)
        assert verify(e, setup, c, z, y, p) is True
        for which in (0, 1):
            zy = [z.copy(), y.copy()]
            zy[which][1] = rows([to_int(zy[which][1]) + R])[0]
            assert verify(e, setup, c, zy[0], zy[1], p) is False              # a RESULT, not an error
        m64 = np.uint64(0xFFFFFFFFFFFFFFFF)
        for which in (0, 1):
            cp = [c.copy(), p.copy()]
            cp[which].reshape(-1, 6)[-1] = m64                               # the last Fp of the array >= p
            with pytest.raises(ZkpError) as ei:
                verify(e, setup, cp[0], z, y, cp[1])
            assert ei.value.status == -4, which
        for which in range(3):
            k = [v.copy() for v in setup.arrays()]
            k[which].reshape(-1, 6)[-1] = m64
            with pytest.raises(ZkpError) as ei:
                verify(e, KzgSetup(*k), c, z, y, p)
            assert ei.value.status == -4, which
    finally:
        e.close()


def test_bad_arguments_at_each_limit(eng):
    from zkvm_pairings_amd import _lib
    lib, h = eng._lib, eng._h
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    res = ctypes.c_int(0)

    def call(n, flags=0, drop_vk=None, drop_b=None, rand=p, out=True, vk_null=False, b_null=False):
        kv = _lib.KzgVk(g1=p, g2=p, tau_g2=p)
        bt = _lib.KzgBatch(n=n, c=p, proof=p, z=p, y=p)
        if drop_vk:
            setattr(kv, drop_vk, None)
        if drop_b:
            setattr(bt, drop_b, None)
        host = lib.zkp_kzg_verify_batch(h, None if vk_null else ctypes.byref(kv), None if b_null else ctypes.byref(bt), rand, flags,
                                        ctypes.byref(res) if out else None)
        dev = lib.zkp_kzg_verify_batch_dev(h, None if vk_null else ctypes.byref(kv), None if b_null else ctypes.byref(bt), rand, flags,
                                           p if out else None, None)
        assert host == dev
        return host

    # every one of these is refused before a byte is read
    assert call((1 << 22) + 1) == -1                          # n > 2^22
    for flags in (4, 8, 7, -1):
        assert call(1, flags=flags) == -1                     # unknown flags
    for f in ("g1", "g2", "tau_g2"):
        assert call(1, drop_vk=f) == -1, f                    # null pointers with non-zero counts
    for f in ("c", "proof", "z", "y"):
        assert call(1, drop_b=f) == -1, f
    assert call(1, rand=None) == -1 and call(1, out=False) == -1 and call(1, vk_null=True) == -1 and call(1, b_null=True) == -1
    assert call(0, flags=4) == -1                             # the limits hold for an empty batch too
    kv, bt = _lib.KzgVk(), _lib.KzgBatch(n=0)                 # inside the limits an empty batch needs no pointers
    assert lib.zkp_kzg_verify_batch(h, ctypes.byref(kv), ctypes.byref(bt), None, 3, ctypes.byref(res)) == 0 and res.value == 1


@pytest.mark.parametrize("log2_n", [6, 12])
def test_blob_batch_a_valid_batch_passes_and_a_changed_evaluation_fails(eng, log2_n):
    from zkvm_pairings_amd import KzgSetup, kzg_verify_blob_batch, synthetic
    n = 3
    setup, ev, c, z, y, p = synthetic.kzg_blob_instance(0xB10B + log2_n, n, log2_n, engine=eng)
    setup = KzgSetup(*setup)
    assert np.array_equal(eng.fr_eval(ev, z, log2_n, bitrev=True), y)
    assert verify(eng, setup, c, z, y, p) is True
    assert kzg_verify_blob_batch(setup, ev, c, z, p, engine=eng) is True
    for j, i in ((0, 0), (1, (1 << log2_n) // 2), (2, (1 << log2_n) - 1)):
        bad = ev.copy()
        bad[j, i] = rows([(to_int(bad[j, i]) + 1) % R])[0]
        assert kzg_verify_blob_batch(setup, bad, c, z, p, engine=eng) is False, (j, i)
    assert kzg_verify_blob_batch(setup, ev, c, z, p, bitrev=False, engine=eng) is (log2_n == 0)     # the order matters
