"""Fr arithmetic on one MI355X (run with -m gpu): every zkp_fr_op_batch operation, zkp_fr_from_wide_batch and zkp_fr_fold_batch, host and
_dev flavours, ragged sizes, operands at the bound, validation mode and bad arguments.  Expected values are Python integers - never the
library under test."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
M64 = (1 << 64) - 1
RAGGED = [1, 63, 64, 65, 1000, (1 << 16) + 3]
EDGE = [0, 1, 2, R - 1, R - 2, 1 << 32, (1 << 32) - 1, 1 << 64, (1 << 128) - 1, 1 << 254, R - (1 << 200), pow(2, 256, R), pow(2, 512, R)]


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(a).reshape(-1, 4)]


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def operands(rng, n):
    v = [rng.randrange(R) for _ in range(n)]
    for i, e in enumerate(EDGE[:n]):
        v[(i * 7) % n] = e
    return v


WANT = {"mul": lambda a, b: a * b % R, "add": lambda a, b: (a + b) % R, "sub": lambda a, b: (a - b) % R, "neg": lambda a, b: -a % R,
        "square": lambda a, b: a * a % R, "invert": lambda a, b: pow(a, R - 2, R)}


@pytest.mark.parametrize("n", RAGGED)
def test_every_op_host_and_dev(eng, n):
    rng = random.Random(0xF100 + n)
    a, b = operands(rng, n), operands(random.Random(n), n)[::-1]
    ra, rb = rows(a), rows(b)
    ta, tb = dev(ra), dev(rb)
    for op, f in WANT.items():
        unary = op in ("neg", "square", "invert")
        want = [f(x, y) for x, y in zip(a, b)]
        got = ints(eng.fr_op(op, ra, None if unary else rb))
        assert got == want, (op, n)
        got = ints(host(eng.fr_op(op, ta, None if unary else tb)))
        assert got == want, (op, n, "dev")
    assert ints(eng.fr_op("invert", rows([0])))[0] == 0


@pytest.mark.parametrize("n", RAGGED)
def test_from_wide_host_and_dev(eng, n):
    rng = random.Random(0xF200 + n)
    vals = [rng.getrandbits(512) for _ in range(n)]
    for i, e in enumerate([0, 1, R, R - 1, (1 << 512) - 1, (1 << 256) - 1, 1 << 256, (R - 1) ** 2][:n]):
        vals[(i * 5) % n] = e
    raw = np.frombuffer(b"".join(v.to_bytes(64, "little") for v in vals), dtype=np.uint8).copy()
    want = [v % R for v in vals]
    assert ints(eng.fr_from_wide(raw)) == want
    assert ints(host(eng.fr_from_wide(dev(raw)))) == want
    if n > 1:                                           # a resident slice that is not 8-byte aligned
        t = dev(np.concatenate([np.zeros(3, dtype=np.uint8), raw]))[3:]
        assert ints(host(eng.fr_from_wide(t))) == want


def test_from_wide_python_class(eng):
    from zkvm_pairings_amd import Fr
    v = (1 << 511) + 12345
    assert int(Fr.from_bytes_wide(v.to_bytes(64, "little"), eng)) == v % R
    assert [int(x) for x in Fr.batch("mul", [3, R - 1], [5, R - 1], eng)] == [15, 1]
    out, sw = Fr.fold([2, 3], [[5, 7], [11, 13]], eng)
    assert [int(x) for x in out] == [43, 53] and int(sw) == 5


POOL = 64


def fold_case(rng, n, l):
    """(w rows, x rows (n, l, 4), expected out, expected sum_w); large cases draw x from a pool of 64 values placed by (7 c + 13 i) % 64, so
    that the expectation is 64 class sums of w times the pool - still exact integers, computed without the library"""
    w = operands(rng, n) if n else []
    if n * l <= 200000:
        x = [[rng.randrange(R) for _ in range(l)] for _ in range(n)]
        for c in range(min(n, 3)):
            for i in range(min(l, 3)):
                x[c][i] = EDGE[(3 * c + i) % len(EDGE)]
        xr = rows([v for row in x for v in row]).reshape(n, l, 4) if n * l else np.zeros((n, l, 4), dtype=np.uint64)
        want = [sum(w[c] * x[c][i] for c in range(n)) % R for i in range(l)]
    else:
        pool = [rng.randrange(R) for _ in range(POOL - 2)] + [R - 1, 0]
        idx = (7 * np.arange(n, dtype=np.int64)[:, None] + 13 * np.arange(l, dtype=np.int64)[None, :]) % POOL
        xr = rows(pool)[idx]
        cls = [sum(w[q::POOL]) for q in range(POOL)]
        want = [sum(cls[q] * pool[(7 * q + 13 * i) % POOL] for q in range(POOL)) % R for i in range(l)]
    return rows(w) if n else np.zeros((0, 4), dtype=np.uint64), xr, want, sum(w) % R


@pytest.mark.parametrize("l", [0, 1, 3, 64, 1000])
@pytest.mark.parametrize("n", [0] + RAGGED)
def test_fold_host_and_dev(eng, n, l):
    w, x, want, want_sw = fold_case(random.Random(0xF300 + 1009 * n + l), n, l)
    out, sw = eng.fr_fold(w, x, l)
    assert ints(out) == want and ints(sw) == [want_sw], (n, l)
    if n:
        out, sw = eng.fr_fold(dev(w), dev(x.reshape(-1, 4)), l)
        assert ints(host(out)) == want and ints(host(sw)) == [want_sw], (n, l, "dev")


@pytest.mark.parametrize("n,l", [(1, 1), (65, 3), ((1 << 16) + 3, 3), (1000, 64), ((1 << 16) + 3, 64)])
def test_fold_with_every_operand_at_r_minus_one(eng, n, l):
    w = np.tile(rows([R - 1]), (n, 1))
    x = np.tile(rows([R - 1]), (n * l, 1))
    out, sw = eng.fr_fold(w, x, l)
    assert ints(out) == [n * (R - 1) ** 2 % R] * l and ints(sw) == [n * (R - 1) % R]
    out, sw = eng.fr_fold(dev(w), dev(x), l)
    assert ints(host(out)) == [n * (R - 1) ** 2 % R] * l and ints(host(sw)) == [n * (R - 1) % R]


def test_fold_is_capturable_and_replays(eng):
    import torch
    w, x, want, want_sw = fold_case(random.Random(0xF400), 1000, 64)
    tw, tx = dev(w), dev(x.reshape(-1, 4))
    eng.fr_fold(tw, tx, 64)                               # grows the workspace outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, sw = eng.fr_fold(tw, tx, 64)
    out.zero_()
    sw.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert ints(host(out)) == want and ints(host(sw)) == [want_sw]


def test_validation_mode_on_non_canonical_limbs(eng):
    from zkvm_pairings_amd import PairingEngine, ZkpError
    e = PairingEngine(0, validate=True)
    try:
        good = rows([5, 7, R - 1])
        for bad_val in (R, R + 1, (1 << 256) - 1):
            bad = rows([5, bad_val, 3])
            for call in (lambda: e.fr_op("mul", bad, good), lambda: e.fr_op("add", good, bad), lambda: e.fr_op("neg", bad),
                         lambda: e.fr_fold(bad, good, 1), lambda: e.fr_fold(good, bad, 1)):
                with pytest.raises(ZkpError) as ei:
                    call()
                assert ei.value.status == -4
        assert ints(e.fr_op("mul", good, good)) == [25, 49, 1]            # canonical operands pass, r - 1 included
        assert ints(e.fr_op("neg", good, None)) == [R - 5, R - 7, 1]
        # unary operations do not read b: garbage there is no error
        assert ints(e.fr_op("square", good, rows([R, R, R]))) == [25, 49, 1]
        # the _dev flavour ORs into the context's word
        assert e.take_validation_status() is False
        e.fr_op("mul", dev(good), dev(good))
        assert e.take_validation_status() is False
        e.fr_op("mul", dev(good), dev(rows([1, 2, R])))
        assert e.take_validation_status() is True
        assert e.take_validation_status() is False
        e.fr_fold(dev(good), dev(rows([1, R, 2])), 1)
        assert e.take_validation_status() is True
        e.fr_fold(dev(rows([1, R, 2])), dev(good), 1)
        assert e.take_validation_status() is True
    finally:
        e.close()
    # validation off: no error
    eng.fr_op("add", rows([R]), rows([1]))


def test_bad_arguments(eng):
    lib, h = eng._lib, eng._h
    buf = np.zeros(64, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    for op in (-1, 6, 16):
        assert lib.zkp_fr_op_batch(h, op, p, p, 1, p) == -1
        assert lib.zkp_fr_op_batch_dev(h, op, p, p, 1, p, None) == -1
    assert lib.zkp_fr_op_batch(h, 0, p, None, 1, p) == -1               # a binary operation without b
    assert lib.zkp_fr_op_batch(h, 0, None, p, 1, p) == -1 and lib.zkp_fr_op_batch(h, 0, p, p, 1, None) == -1
    assert lib.zkp_fr_op_batch(h, 3, p, None, 1, p) == 0                # neg ignores b
    assert lib.zkp_fr_op_batch(h, 0, None, None, 0, None) == 0
    assert lib.zkp_fr_from_wide_batch(h, None, 1, p) == -1 and lib.zkp_fr_from_wide_batch(h, p, 1, None) == -1
    assert lib.zkp_fr_from_wide_batch(h, None, 0, None) == 0
    # the fold's limits: refused before anything is read
    for n, l in (((1 << 24) + 1, 1), (1, 65536), (1 << 16, 1 << 15), ((1 << 24), 128)):
        assert lib.zkp_fr_fold_batch(h, p, p, n, l, p, p) == -1, (n, l)
        assert lib.zkp_fr_fold_batch_dev(h, p, p, n, l, p, p, None) == -1, (n, l)
    assert lib.zkp_fr_fold_batch(h, None, p, 1, 1, p, p) == -1 and lib.zkp_fr_fold_batch(h, p, None, 1, 1, p, p) == -1
    assert lib.zkp_fr_fold_batch(h, p, p, 1, 1, None, p) == -1
    out = np.full(8, 7, dtype=np.uint64)
    assert lib.zkp_fr_fold_batch(h, None, None, 0, 1, ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(out[4:].ctypes.data)) == 0   # n == 0: zeros
    assert not out.any()
    assert lib.zkp_fr_fold_batch(h, p, None, 1, 0, None, None) == 0      # nothing to compute
