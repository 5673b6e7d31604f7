"""The batched Fr inversion and the barycentric evaluation on one MI355X (run with -m gpu): bit for bit against Python integers and against
fr_op("invert"), at every size where the kernels take another path (one lane, one run, one workgroup and just past it, a middle level of
one total), with zeros wherever they can sit, in place, host / device / captured-graph flavours, validation mode and the argument limits."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BLOCK = 4 * 256                                               # one thread's run times the workgroup size
INV_NS = [1, 2, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 5000, (1 << 16) + 3]


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(arr):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)]


def inv(v):
    return pow(v, -1, R) if v else 0


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "fr_operands.json")) as f:
        g = json.load(f)
    return sorted({int(g[k], 16) % R for k in ("largest", "fr_r", "fr_r2", "fr_r3")} | {int(v, 16) % R for v in g["from_u512"]})


def operands(n, seed):
    rng = random.Random(seed)
    vals = [rng.randrange(1, R) for _ in range(n)]
    for i, v in enumerate([1, R - 1] + golden()):
        if 2 * i + 1 < n:
            vals[2 * i + 1] = v
    return vals


def tensor(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to("cuda:0")


@pytest.mark.parametrize("n", INV_NS)
def test_inversion_is_bit_equal_to_python_and_to_fr_op(eng, n):
    vals = operands(n, 0x1A0 + n)
    cases = [vals]
    for idx in ([0], [n // 2], [n - 1], list(range(max(0, BLOCK - 3), min(n, BLOCK + 3))), list(range(n))):
        v = list(vals)
        for i in idx:
            v[i] = 0
        cases.append(v)                                        # zeros first, middle, last, across a workgroup boundary, everywhere
    for v in cases:
        a = rows(v)
        got = eng.fr_invert(a)
        assert ints(got) == [inv(x) for x in v]
        assert np.array_equal(got, eng.fr_op("invert", a))


@pytest.mark.parametrize("n", [1, 5, 257, BLOCK + 1, 5000])
def test_in_place_host_device_and_graph_replay_agree(eng, n):
    import torch
    vals = operands(n, 0x1A1 + n)
    vals[n // 2] = 0
    a = rows(vals)
    want = eng.fr_invert(a)
    ta = tensor(a)
    out = eng.fr_invert(ta)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
    tb = ta.clone()
    assert eng.fr_invert(tb, out=tb) is tb                     # in place equals out of place
    torch.cuda.synchronize()
    assert torch.equal(tb, out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gout = eng.fr_invert(ta)
    for _ in range(2):
        gout.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gout, out)


def test_inversion_validation_mode_and_argument_limits(eng):
    from zkvm_pairings_amd import PairingEngine, ZkpError
    e = PairingEngine(0, validate=True)
    try:
        a = rows([5, R - 1, 7])
        assert ints(e.fr_invert(a)) == [inv(5), inv(R - 1), inv(7)]
        for bad in (R, R + 1, (1 << 256) - 1):
            b = a.copy()
            b[1] = rows([bad])[0]
            with pytest.raises(ZkpError) as ei:
                e.fr_invert(b)
            assert ei.value.status == -4
    finally:
        e.close()
    lib, h = eng._lib, eng._h
    buf = np.zeros(8, dtype=np.uint64)
    p = buf.ctypes.data
    assert lib.zkp_fr_invert_batch(h, p, 1 << 31, p) == -1 and lib.zkp_fr_invert_batch_dev(h, p, 1 << 31, p, None) == -1      # n > 2^31 - 1
    assert lib.zkp_fr_invert_batch(h, None, 1, p) == -1 and lib.zkp_fr_invert_batch(h, p, 1, None) == -1
    assert lib.zkp_fr_invert_batch_dev(h, None, 1, p, None) == -1 and lib.zkp_fr_invert_batch_dev(h, p, 1, None, None) == -1
    assert lib.zkp_fr_invert_batch(h, None, 0, None) == 0 and lib.zkp_fr_invert_batch_dev(h, None, 0, None, None) == 0         # n = 0 is legal
    assert eng.fr_invert(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)
    from zkvm_pairings_amd import Fr
    assert [int(v) for v in Fr.invert_batch([3, 0, R - 1], engine=eng)] == [inv(3), 0, R - 1]


# ---- the evaluation
_evals = {}


def poly(log2_n, n_poly):
    """n_poly random evaluation vectors of 2^log2_n values; polynomial 0 is the zero polynomial and the last one a constant when there
    are at least three.  Cached: callers copy what they change."""
    key = (log2_n, n_poly)
    if key not in _evals:
        rng = random.Random(0xE7A + 100 * log2_n + n_poly)
        n = 1 << log2_n
        f = [[rng.randrange(R) for _ in range(n)] for _ in range(n_poly)]
        if n_poly >= 3:
            f[0] = [0] * n
            f[-1] = [f[-1][0]] * n
        _evals[key] = f
    return _evals[key]


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("n_poly", [1, 3, 5])
@pytest.mark.parametrize("log2_n", [0, 1, 2, 6, 8, 9, 12])
def test_evaluation_against_the_python_model(eng, log2_n, n_poly, bitrev):
    import torch
    from zkvm_pairings_amd import synthetic
    rng = random.Random(0xE7B + log2_n)
    n = 1 << log2_n
    f = poly(log2_n, n_poly)
    w = synthetic.fr_root_of_unity(log2_n)
    flat = rows([v for row in f for v in row])
    zsets = [[rng.randrange(R) for _ in range(n_poly)], [0] * n_poly] + [[pow(w, i, R)] * n_poly for i in sorted({0, n // 2, n - 1})]
    te = tensor(flat)
    for zs in zsets:
        want = [synthetic.barycentric_eval(f[j], zs[j], log2_n, bitrev) for j in range(n_poly)]
        z = rows(zs)
        assert ints(eng.fr_eval(flat, z, log2_n, bitrev)) == want
        got = eng.fr_eval(te, tensor(z), log2_n, bitrev)
        torch.cuda.synchronize()
        assert ints(got.cpu().numpy().view(np.uint64)) == want
    if n_poly >= 3:
        assert want[0] == 0 and want[-1] == f[-1][0]          # the zero and the constant polynomial
    if n_poly == 1:
        from zkvm_pairings_amd import Fr
        assert int(Fr.evaluate(f[0], zsets[0][0], bitrev, engine=eng)) == synthetic.barycentric_eval(f[0], zsets[0][0], log2_n, bitrev)


@pytest.mark.parametrize("log2_n,n_poly", [(0, 3), (6, 5), (9, 3)])
def test_evaluation_graph_replay_agrees(eng, log2_n, n_poly):
    import torch
    from zkvm_pairings_amd import synthetic
    rng = random.Random(0xE7C + log2_n)
    f = poly(log2_n, n_poly)
    w = synthetic.fr_root_of_unity(log2_n)
    zs = [rng.randrange(R) for _ in range(n_poly)]
    zs[1] = pow(w, (1 << log2_n) - 1, R)                      # one point in the domain
    want = [synthetic.barycentric_eval(f[j], zs[j], log2_n, True) for j in range(n_poly)]
    te, tz = tensor(rows([v for row in f for v in row])), tensor(rows(zs))
    out = eng.fr_eval(te, tz, log2_n, True)
    torch.cuda.synchronize()
    assert ints(out.cpu().numpy().view(np.uint64)) == want
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gout = eng.fr_eval(te, tz, log2_n, True)
    for _ in range(2):
        gout.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gout, out)


def test_evaluation_limits_and_validation(eng):
    from zkvm_pairings_amd import PairingEngine, ZkpError
    lib, h = eng._lib, eng._h
    buf = np.zeros(8, dtype=np.uint64)
    p = buf.ctypes.data

    def call(n_poly, log2_n, flags=0, evals=p, z=p, out=p):
        host = lib.zkp_fr_eval_batch(h, evals, z, n_poly, log2_n, flags, out)
        dev = lib.zkp_fr_eval_batch_dev(h, evals, z, n_poly, log2_n, flags, out, None)
        assert host == dev
        return host

    # every one of these is refused before a byte is read
    assert call(1, 21) == -1 and call(0, 21) == -1 and call(1, 64) == -1               # log2_n > 20
    assert call((1 << 26) + 1, 0) == -1 and call(65, 20) == -1 and call((1 << 14) + 1, 12) == -1      # n_poly N > 2^26
    for flags in (2, 4, 3, -1):
        assert call(1, 1, flags=flags) == -1                  # unknown flags
    assert call(1, 1, evals=None) == -1 and call(1, 1, z=None) == -1 and call(1, 1, out=None) == -1
    assert call(0, 20, evals=None, z=None, out=None) == 0     # n_poly = 0 is legal
    e = PairingEngine(0, validate=True)
    try:
        f, z = rows([1, 2, 3, 4]), rows([9])
        assert ints(e.fr_eval(f, z, 2)) == [__import__("zkvm_pairings_amd").synthetic.barycentric_eval([1, 2, 3, 4], 9, 2)]
        bad = f.copy()
        bad[3] = rows([R])[0]
        with pytest.raises(ZkpError) as ei:
            e.fr_eval(bad, z, 2)
        assert ei.value.status == -4
        with pytest.raises(ZkpError) as ei:
            e.fr_eval(f, rows([R + 5]), 2)
        assert ei.value.status == -4
    finally:
        e.close()
