"""The batched Groth16 verifier on one MI355X (run with -m gpu): batches from synthetic.groth16_instance, whose verdict is known from how
they are built (secret exponents) - valid batches, bad proofs anywhere, changed and non-canonical public inputs, two bad proofs that
cancel in a plain product, zero scalars, points outside the groups in every position, compressed input, host / device / captured-graph
flavours and bad arguments - and the per-proof path groth16_verify_each, which is composed of calls that do not know Groth16."""
import ctypes
import random

import numpy as np
import pytest

import outside_groups as og

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
NS = [1, 2, 5, 127, 1000]
LS = [0, 1, 3, 64]


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


_cache = {}


def instance(eng, n, l):
    """(vk, (A, B, C), inputs) of a valid batch; cached, callers copy what they change"""
    from zkvm_pairings_amd import Groth16VerifyingKey, synthetic
    if (n, l) not in _cache:
        key, proofs, x = synthetic.groth16_instance(0x616000 + 1000 * l + n, n, l, engine=eng)
        _cache[(n, l)] = (Groth16VerifyingKey(*key), proofs, x)
    return _cache[(n, l)]


def rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def to_int(row):
    return int.from_bytes(np.ascontiguousarray(row).tobytes(), "little")


def g1_times(eng, k):
    from zkvm_pairings_amd import synthetic
    return eng.g1_mul(synthetic.G1_GENERATOR, rows([k % R]))[0][0]


def shifted(eng, c, idx, k=1):
    """C with C[idx] + [k] G1"""
    c = c.copy()
    for i in idx:
        s, inf = eng.g1_add(c[i], g1_times(eng, k))
        assert not inf[0]
        c[i] = s[0]
    return c


def verify(eng, vk, proofs, x, **kw):
    from zkvm_pairings_amd import groth16_verify_batch
    return groth16_verify_batch(vk, proofs, x, engine=eng, **kw)


@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("n", NS)
def test_valid_batches_pass_and_one_bad_proof_fails(eng, n, l):
    vk, (a, b, c), x = instance(eng, n, l)
    assert verify(eng, vk, (a, b, c), x) is True
    assert verify(eng, vk, (a, b, c), x, points_checked=True, vk_checked=True) is True
    for idx in sorted({0, n // 2, n - 1}):                  # first, middle, last
        assert verify(eng, vk, (a, b, shifted(eng, c, [idx])), x) is False, idx
    if l:
        for ci, ii in sorted({(0, 0), (n // 2, l // 2), (n - 1, l - 1)}):
            v = to_int(x[ci, ii])
            y = x.copy()
            y[ci, ii] = rows([(v + 1) % R])[0]                # a changed public input
            assert verify(eng, vk, (a, b, c), y) is False, (ci, ii)
            assert v + R < 1 << 256                           # r < 2^255: x + r always fits
            y[ci, ii] = rows([v + R])[0]                      # the same residue, not the same input
            assert verify(eng, vk, (a, b, c), y) is False, (ci, ii, "x + r")
            assert verify(eng, vk, (a, b, c), y, points_checked=True, vk_checked=True) is False


def test_synthetic_bad_list_marks_exactly_those_proofs(eng):
    from zkvm_pairings_amd import Groth16VerifyingKey, groth16_verify_each, synthetic
    n, l = 9, 3
    key, proofs, x = synthetic.groth16_instance(0xBAD, n, l, bad=(0, 4, 8), engine=eng)
    vk = Groth16VerifyingKey(*key)
    assert verify(eng, vk, proofs, x) is False
    each = groth16_verify_each(vk, proofs, x, engine=eng)
    assert each.tolist() == [i not in (0, 4, 8) for i in range(n)]
    key2, proofs2, x2 = synthetic.groth16_instance(0xBAD, n, l, engine=eng)
    assert np.array_equal(proofs2[2], shifted(eng, proofs[2], [0, 4, 8], k=R - 1)) and np.array_equal(x, x2)
    assert verify(eng, Groth16VerifyingKey(*key2), proofs2, x2) is True


@pytest.mark.parametrize("n,l", [(2, 0), (5, 3), (127, 1), (1000, 64)])
def test_two_bad_proofs_that_cancel_in_a_plain_product_fail(eng, n, l):
    vk, (a, b, c), x = instance(eng, n, l)
    i, j = 0, n - 1
    bad = shifted(eng, shifted(eng, c, [i], k=17), [j], k=R - 17)     # C_i + D, C_j - D: e(C_i + D, delta) e(C_j - D, delta) is unchanged
    assert verify(eng, vk, (a, b, bad), x) is False
    # with equal scalars on the two proofs the combination cannot tell - this is why the scalars are random: the check itself
    rand = eng.rlc_random(n)
    rand[j] = rand[i]
    assert verify(eng, vk, (a, b, bad), x, rand=rand) is True


def test_zero_scalars_fail(eng):
    for n, l in ((1, 0), (5, 3), (127, 1)):
        vk, proofs, x = instance(eng, n, l)
        for idx in sorted({0, n // 2, n - 1}):
            rand = eng.rlc_random(n)
            rand[idx] = 0
            assert verify(eng, vk, proofs, x, rand=rand) is False
            assert verify(eng, vk, proofs, x, rand=rand, points_checked=True, vk_checked=True) is False
        rand = eng.rlc_random(n)
        rand[:, 1] = 0                                        # (a, 0) and (0, b) are legal scalars
        assert verify(eng, vk, proofs, x, rand=rand) is True
        rand = eng.rlc_random(n)
        rand[:, 0] = 0
        assert verify(eng, vk, proofs, x, rand=rand) is True


def test_points_outside_the_groups_fail_in_every_position(eng):
    from zkvm_pairings_amd import Groth16VerifyingKey
    n, l = 2, 1
    vk, (a, b, c), x = instance(eng, n, l)
    g1s = {k: og.g1_wire(p) for k, p in og.g1_points().items()}
    g2s = {k: og.g2_wire(q) for k, q in og.g2_points().items()}
    assert len(g1s) >= 2 and len(g2s) >= 2
    assert eng.g1_is_valid(np.stack(list(g1s.values()))).all() and eng.g2_is_valid(np.stack(list(g2s.values()))).all()   # none of them is valid
    for name, p in g1s.items():
        for pos in range(n):
            for which in (0, 2):
                pr = [a.copy(), b, c.copy()]
                pr[which][pos] = p
                assert verify(eng, vk, tuple(pr), x) is False, (name, pos, which)
        assert verify(eng, Groth16VerifyingKey(p, vk.beta_g2, vk.gamma_g2, vk.delta_g2, vk.ic), (a, b, c), x) is False, name
        for pos in range(l + 1):
            ic = vk.ic.copy()
            ic[pos] = p
            assert verify(eng, Groth16VerifyingKey(vk.alpha_g1, vk.beta_g2, vk.gamma_g2, vk.delta_g2, ic), (a, b, c), x) is False, (name, pos)
    for name, q in g2s.items():
        for pos in range(n):
            bb = b.copy()
            bb[pos] = q
            assert verify(eng, vk, (a, bb, c), x) is False, (name, pos)
        for pos in range(3):
            g2 = [vk.beta_g2, vk.gamma_g2, vk.delta_g2]
            g2[pos] = q
            assert verify(eng, Groth16VerifyingKey(vk.alpha_g1, *g2, vk.ic), (a, b, c), x) is False, (name, pos)
    # a flagged infinity is a valid point, but no proof with one verifies against this key
    assert eng.groth16_verify_batch(*vk.arrays(), a, b, c, x, inf_a=np.array([1, 0], dtype=np.uint8)) is False


def test_empty_batch_passes(eng):
    from zkvm_pairings_amd import _lib
    vk, _, _ = instance(eng, 1, 3)
    assert verify(eng, vk, (np.zeros((0, 12)), np.zeros((0, 24)), np.zeros((0, 12))), None) is True
    res = ctypes.c_int(5)
    kv, bt = _lib.Groth16Vk(n_inputs=3), _lib.Groth16Batch(n=0)
    assert eng._lib.zkp_groth16_verify_batch(eng._h, ctypes.byref(kv), ctypes.byref(bt), None, 0, ctypes.byref(res)) == 0 and res.value == 1
    import torch
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
    assert eng._lib.zkp_groth16_verify_batch_dev(eng._h, ctypes.byref(kv), ctypes.byref(bt), None, 0, ctypes.c_void_p(flag.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 1


@pytest.mark.parametrize("n,l,seed", [(5, 0, 1), (5, 3, 2), (127, 1, 3), (127, 64, 4), (1000, 3, 5)])
def test_batch_verdict_equals_all_of_verify_each_on_mixed_batches(eng, n, l, seed):
    from zkvm_pairings_amd import groth16_verify_each
    rng = random.Random(0xEAC0 + seed)
    vk, (a, b, c), x = instance(eng, n, l)
    each = groth16_verify_each(vk, (a, b, c), x, engine=eng)
    assert each.all() and verify(eng, vk, (a, b, c), x) is True
    for trial in range(3):
        bad_c = sorted(rng.sample(range(n), rng.choice([0, 1, 2])))
        bad_x = sorted(rng.sample(range(n), rng.choice([0, 1]))) if l else []
        non_canonical = sorted(rng.sample(range(n), rng.choice([0, 1]))) if l else []
        cc, y = shifted(eng, c, bad_c, k=rng.randrange(1, R)), x.copy()
        for i in bad_x:
            y[i, rng.randrange(l)] = rows([rng.randrange(R)])[0]
        for i in non_canonical:
            j = rng.randrange(l)
            y[i, j] = rows([to_int(y[i, j]) + R])[0]
        want = [i not in bad_c and i not in bad_x and i not in non_canonical for i in range(n)]     # by construction
        each = groth16_verify_each(vk, (a, b, cc), y, engine=eng)
        assert each.tolist() == want, trial
        assert verify(eng, vk, (a, b, cc), y) is all(want), trial


def test_compressed_input_agrees_with_point_input(eng):
    from zkvm_pairings_amd import groth16_verify_each
    n, l = 127, 3
    vk, (a, b, c), x = instance(eng, n, l)

    def packed(a, b, c):
        ca = np.frombuffer(eng.compress_points(a, 1), dtype=np.uint8).reshape(n, 48)
        cb = np.frombuffer(eng.compress_points(b, 2), dtype=np.uint8).reshape(n, 96)
        cc = np.frombuffer(eng.compress_points(c, 1), dtype=np.uint8).reshape(n, 48)
        return np.ascontiguousarray(np.concatenate([ca, cb, cc], axis=1))

    raw = packed(a, b, c)
    assert raw.shape == (n, 192)
    assert verify(eng, vk, raw, x) is True and groth16_verify_each(vk, raw, x, engine=eng).all()
    bad = shifted(eng, c, [60])
    raw_bad = packed(a, b, bad)
    assert verify(eng, vk, raw_bad, x) is verify(eng, vk, (a, b, bad), x) is False
    assert groth16_verify_each(vk, raw_bad, x, engine=eng).tolist() == [i != 60 for i in range(n)]
    # a proof that fails to decompress fails the batch: the compression flag cleared, and an x with no point on the curve
    for col in (0, 48, 144):
        broken = raw.copy()
        broken[7, col] &= 0x7F
        assert verify(eng, vk, broken, x) is False
        assert groth16_verify_each(vk, broken, x, engine=eng).tolist() == [i != 7 for i in range(n)]
    found = False
    for t in range(1, 40):
        cand = raw.copy()
        cand[3, 47] = (int(cand[3, 47]) + t) & 0xFF          # another x for A_3: about half of them are on no point
        _, _, st = eng.decompress_points(np.ascontiguousarray(cand[3, :48]), 1)
        if st[0] == 3:
            assert verify(eng, vk, cand, x) is False
            found = True
            break
    assert found


def tensors(eng, vk, proofs, x):
    import torch
    d = torch.device("cuda", 0)
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to(d)
    return [t(v) for v in vk.arrays()], [t(p) for p in proofs], t(x.reshape(-1, 4))


@pytest.mark.parametrize("n,l", [(1, 0), (5, 3), (127, 64)])
def test_host_dev_and_graph_replay_agree(eng, n, l):
    import torch
    vk, (a, b, c), x = instance(eng, n, l)
    for proofs, want in (((a, b, c), True), ((a, b, shifted(eng, c, [n // 2])), False)):
        rand = eng.rlc_random(n)
        assert eng.groth16_verify_batch(*vk.arrays(), *proofs, x, rand=rand) is want
        tk, tp, tx = tensors(eng, vk, proofs, x)
        tr = torch.from_numpy(rand.view(np.int64)).to(tx.device)
        got = eng.groth16_verify_batch(*tk, *tp, tx, rand=tr)
        torch.cuda.synchronize()
        assert got.dtype == torch.int32 and bool(got.item()) is want
        for kw in ({}, {"points_checked": True, "vk_checked": True}):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gflag = eng.groth16_verify_batch(*tk, *tp, tx, rand=tr, **kw)
            gflag.fill_(7)
            graph.replay()
            torch.cuda.synchronize()
            assert int(gflag.item()) == int(want)
            gflag.fill_(7)
            graph.replay()
            torch.cuda.synchronize()
            assert int(gflag.item()) == int(want)


def test_validation_mode_keeps_the_rule_for_coordinates_and_not_for_inputs(eng):
    from zkvm_pairings_amd import Groth16VerifyingKey, PairingEngine, ZkpError
    e = PairingEngine(0, validate=True)
    try:
        n, l = 2, 1
        vk, (a, b, c), x = instance(eng, n, l)
        assert verify(e, vk, (a, b, c), x) is True
        y = x.copy()
        y[1, 0] = rows([to_int(x[1, 0]) + R])[0]
        assert verify(e, vk, (a, b, c), y) is False                    # a RESULT, not an error
        m64 = np.uint64(0xFFFFFFFFFFFFFFFF)
        for which in range(3):
            pr = [a.copy(), b.copy(), c.copy()]
            pr[which].reshape(-1, 6)[-1] = m64                           # the last Fp of the array >= p
            with pytest.raises(ZkpError) as ei:
                verify(e, vk, tuple(pr), x)
            assert ei.value.status == -4, which
        for which in range(5):
            k = [v.copy() for v in vk.arrays()]
            k[which].reshape(-1, 6)[-1] = m64
            with pytest.raises(ZkpError) as ei:
                verify(e, Groth16VerifyingKey(*k), (a, b, c), x)
            assert ei.value.status == -4, which
    finally:
        e.close()


def test_bad_arguments_at_each_limit(eng):
    from zkvm_pairings_amd import _lib
    lib, h = eng._lib, eng._h
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    res = ctypes.c_int(0)

    def call(n, l, flags=0, drop_vk=None, drop_b=None, rand=p, out=True, vk_null=False, b_null=False):
        kv = _lib.Groth16Vk(alpha_g1=p, beta_g2=p, gamma_g2=p, delta_g2=p, n_inputs=l, ic=p)
        bt = _lib.Groth16Batch(n=n, a=p, b=p, c=p, inputs=p)
        if drop_vk:
            setattr(kv, drop_vk, None)
        if drop_b:
            setattr(bt, drop_b, None)
        host = lib.zkp_groth16_verify_batch(h, None if vk_null else ctypes.byref(kv), None if b_null else ctypes.byref(bt), rand, flags,
                                            ctypes.byref(res) if out else None)
        dev = lib.zkp_groth16_verify_batch_dev(h, None if vk_null else ctypes.byref(kv), None if b_null else ctypes.byref(bt), rand, flags,
                                               p if out else None, None)
        assert host == dev
        return host

    # every one of these is refused before a byte is read
    assert call((1 << 24) + 1, 0) == -1                       # n > 2^24
    assert call(1, 65536) == -1                               # n_inputs > 65535
    assert call(1 << 16, 1 << 15) == -1                       # n n_inputs = 2^31 > 2^31 - 1
    assert call(1 << 24, 128) == -1
    for flags in (4, 8, 7, -1):
        assert call(1, 1, flags=flags) == -1                  # unknown flags
    for f in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "ic"):
        assert call(1, 1, drop_vk=f) == -1, f                 # null pointers with non-zero counts
    for f in ("a", "b", "c", "inputs"):
        assert call(1, 1, drop_b=f) == -1, f
    assert call(1, 1, rand=None) == -1 and call(1, 1, out=False) == -1 and call(1, 1, vk_null=True) == -1 and call(1, 1, b_null=True) == -1
    assert call(0, 65536) == -1 and call(0, 0, flags=4) == -1     # the limits hold for an empty batch too
    # inside the limits an empty batch needs no pointers
    kv, bt = _lib.Groth16Vk(n_inputs=65535), _lib.Groth16Batch(n=0)
    assert lib.zkp_groth16_verify_batch(h, ctypes.byref(kv), ctypes.byref(bt), None, 3, ctypes.byref(res)) == 0 and res.value == 1
    # n_inputs == 0 needs no inputs pointer: vk_x = IC_0
    vk, (a, b, c), x = instance(eng, 2, 0)
    assert eng.groth16_verify_batch(*vk.arrays(), a, b, c, None) is True


@pytest.mark.parametrize("m,n_msm", [(1, 1), (5, 1), (127, 1), (4, 2), (65, 2), (1000, 3)])
def test_a_captured_msm_replays_more_than_once(eng, m, n_msm):
    """the verifier's two MSM calls sit inside its captured call: a captured MSM gives the eager sums on EVERY replay, not only the first"""
    import torch
    from zkvm_pairings_amd import synthetic
    rng = random.Random(0x6A70 + 7 * m + n_msm)
    d = torch.device("cuda", 0)
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to(d)
    pts = t(eng.g1_mul(synthetic.G1_GENERATOR, rows([rng.randrange(1, R) for _ in range(m * n_msm)]))[0])
    sc = t(rows([rng.randrange(R) for _ in range(m * n_msm)]))
    want, want_inf = eng.g1_msm(pts, sc, n_msm)
    torch.cuda.synchronize()
    want, want_inf = want.clone(), want_inf.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, inf = eng.g1_msm(pts, sc, n_msm)
    for replay in range(4):
        out.fill_(7)
        inf.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(inf, want_inf), replay
