"""The batched Fr NTT (zkp_fr_ntt_batch, include/zkp_poly.h) on one MI355X against tests/poly_model.py (Python integers), byte for byte:
every size from one element to the first two-pass sizes, all eight flag combinations, the host flavour, the device flavour and in
place; adversarial operands; the large sizes up to the first three-pass plans and the ABI maximum; its agreement with fr_eval; a growing
domain table; validation mode; argument errors.  Run with -m gpu.

The tile holds 2^10 elements: 9, 10, 11 are in the range of the first test; the first three-pass sizes are 2^17 (natural order) and
2^19 (ZKP_NTT_BITREV), both among the large sizes."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import poly_model as pm
from replay_cases import fr_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = pm.R
FLAGS = range(8)


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def kw(flags):
    return dict(inverse=bool(flags & pm.INVERSE), bitrev=bool(flags & pm.BITREV), coset=bool(flags & pm.COSET))


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def rows_bytes(ints):
    return b"".join(v.to_bytes(32, "little") for v in ints)


def check_all_flavours(eng, x, want, log2_n, flags, what):
    """x, want: (n, 4) uint64"""
    wb = want.tobytes()
    assert eng.fr_ntt(x, log2_n, **kw(flags)).tobytes() == wb, (what, "host")
    buf = x.copy()
    assert eng.fr_ntt(buf, log2_n, out=buf, **kw(flags)) is buf and buf.tobytes() == wb, (what, "host in place")
    t = to_dev(x)
    assert eng.fr_ntt(t, log2_n, **kw(flags)).cpu().numpy().tobytes() == wb, (what, "dev")
    assert t.cpu().numpy().tobytes() == x.tobytes(), (what, "dev: the input changed")
    assert eng.fr_ntt(t, log2_n, out=t, **kw(flags)) is t and t.cpu().numpy().tobytes() == wb, (what, "dev in place")


def model_pairs(polys, log2_n):
    """flags -> (inputs, outputs) per polynomial.  The forward maps come from the model; an inverse map's input is the forward map's
    output and its output the coefficients (tests/test_poly_cpu.py holds the model to that on its own)"""
    out = {}
    for flags in (0, pm.BITREV, pm.COSET, pm.BITREV | pm.COSET):
        fwd = [pm.ntt_flags(p, log2_n, flags) for p in polys]
        out[flags] = (polys, fwd)
        out[flags | pm.INVERSE] = (fwd, polys)
    return out


@pytest.mark.parametrize("log2_n", range(14))
def test_ntt_against_the_model(eng, log2_n):
    rng = random.Random(0x177 + log2_n)
    n = 1 << log2_n
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(5)]
    pairs = model_pairs(polys, log2_n)
    if log2_n <= 6:                                     # the inverse from the model itself as well, where that is cheap
        for flags in (1, 3, 5, 7):
            assert [pm.ntt_flags(p, log2_n, flags) for p in pairs[flags][0]] == polys
    for flags in FLAGS:
        src, dst = pairs[flags]
        for n_poly in (1, 3, 5):
            x = fr_rows([v for p in src[:n_poly] for v in p])
            want = fr_rows([v for p in dst[:n_poly] for v in p])
            check_all_flavours(eng, x, want, log2_n, flags, (log2_n, flags, n_poly))


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "fr_operands.json")) as f:
        g = json.load(f)
    vals = [int(g[k], 16) for k in ("largest", "fr_r", "fr_r2", "fr_r3")] + [int(v, 16) for v in g["from_u512"]]
    return sorted(set(v % R for v in vals))


@pytest.mark.parametrize("log2_n", [0, 1, 2, 5, 10, 11])
def test_ntt_on_adversarial_operands(eng, log2_n):
    """all r - 1, all zero, a delta at 0, 1, N/2, N/2 + 1, N - 1 (its transform is the k-th powers of the whole domain: every twiddle
    index is read), the stored operands of tests/golden and values with a full top limb"""
    n = 1 << log2_n
    gold = _golden()
    top = [R - 1, R - 2, R - (1 << 64), (R >> 192) << 192, ((R >> 192) << 192) | 1]          # the top limb is r's own
    polys = [[R - 1] * n, [0] * n, [gold[i % len(gold)] for i in range(n)], [top[i % len(top)] for i in range(n)]]
    for k in sorted(set(k for k in (0, 1, n // 2, n // 2 + 1, n - 1) if 0 <= k < n)):
        polys.append([R - 1 if i == k else 0 for i in range(n)])
    for flags in FLAGS:
        want = [pm.ntt_flags(p, log2_n, flags) for p in polys]
        if not flags & pm.INVERSE and log2_n <= 5:
            assert want[0] == pm.ntt_definition(polys[0], log2_n, **{k: v for k, v in kw(flags).items() if k != "inverse"})
        x, w = fr_rows([v for p in polys for v in p]), fr_rows([v for p in want for v in p])
        assert eng.fr_ntt(x, log2_n, **kw(flags)).tobytes() == w.tobytes(), (log2_n, flags)
        t = to_dev(x)
        assert eng.fr_ntt(t, log2_n, out=t, **kw(flags)).cpu().numpy().tobytes() == w.tobytes(), (log2_n, flags, "dev")


_DOMAIN = {}


def _domain(log2_n):
    if log2_n not in _DOMAIN:
        _DOMAIN[log2_n] = pm.domain(log2_n)
    return _DOMAIN[log2_n]


def sparse_expected(log2_n, c0, c1, ca, cb, bitrev, coset):
    """the transform of c0 + c1 X + ca X^(N/2+1) + cb X^(N-1): at x = s w^i the powers are s w^i, -+ s^(N/2+1) w^i and s^(N-1) w^-i"""
    n = 1 << log2_n
    d = _domain(log2_n)
    s = pm.GENERATOR if coset else 1
    c1, ca, cb = c1 * s % R, ca * pow(s, n // 2 + 1, R) % R, cb * pow(s, n - 1, R) % R
    even, odd = (c1 + ca) % R, (c1 - ca) % R
    nat = [(c0 + d[i] * (odd if i & 1 else even) + cb * d[(n - i) & (n - 1)]) % R for i in range(n)]
    if not bitrev:
        return nat
    shift = 32 - log2_n
    idx = np.arange(n, dtype=np.uint32)
    for sh, m in ((1, 0x55555555), (2, 0x33333333), (4, 0x0F0F0F0F), (8, 0x00FF00FF)):
        idx = ((idx >> sh) & m) | ((idx & m) << sh)
    idx = ((idx >> 16) | (idx << 16)) >> shift
    return [nat[int(j)] for j in idx]


@pytest.mark.parametrize("log2_n,flags", [(16, 0), (16, 2), (16, 4), (16, 6), (17, 0), (17, 4), (19, 2), (19, 6), (20, 0), (20, 6)])
def test_ntt_large_sparse(eng, log2_n, flags):
    """at most four non-zero coefficients, at 0, 1, N/2 + 1 and N - 1: the whole expected vector from a Python domain table.  2^16: the
    last two-pass size in natural order; 2^17 and 2^19: the first three-pass sizes; 2^20: the ABI maximum"""
    rng = random.Random(0x5A + log2_n + flags)
    n = 1 << log2_n
    c0, c1, ca, cb = (rng.randrange(1, R) for _ in range(4))
    want = rows_bytes(sparse_expected(log2_n, c0, c1, ca, cb, bool(flags & pm.BITREV), bool(flags & pm.COSET)))
    x = np.zeros((n, 4), dtype=np.uint64)
    for k, c in ((0, c0), (1, c1), (n // 2 + 1, ca), (n - 1, cb)):
        x[k] = fr_rows([c])[0]
    t = to_dev(x)
    got = eng.fr_ntt(t, log2_n, **kw(flags))
    assert got.cpu().numpy().tobytes() == want
    # and back, in place
    back = eng.fr_ntt(got, log2_n, out=got, **kw(flags | pm.INVERSE))
    assert back.cpu().numpy().tobytes() == x.tobytes()


def _dense(n, seed):
    """n canonical elements: random words, the top one below 2^62"""
    x = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    x[:, 3] >>= np.uint64(2)
    return x


@pytest.mark.parametrize("log2_n", [16, 17, 19, 20])
def test_ntt_large_dense_round_trip(eng, log2_n):
    x = _dense(1 << log2_n, log2_n)
    t = to_dev(x)
    for flags in (0, pm.BITREV, pm.COSET, pm.BITREV | pm.COSET):
        fwd = eng.fr_ntt(t, log2_n, **kw(flags))
        assert fwd.cpu().numpy().tobytes() != x.tobytes()
        assert eng.fr_ntt(fwd, log2_n, **kw(flags | pm.INVERSE)).cpu().numpy().tobytes() == x.tobytes(), (log2_n, flags)
        # the inverse first: it is a bijection as well
        inv = eng.fr_ntt(t, log2_n, **kw(flags | pm.INVERSE))
        assert eng.fr_ntt(inv, log2_n, out=inv, **kw(flags)).cpu().numpy().tobytes() == x.tobytes(), (log2_n, flags, "inverse first")


def horner8(coeffs, z0):
    """f at the eight points z0 u^j, u the 8th root of unity: all eight share (z0 u^j)^8 = z0^8, so one Horner run in z0^8 over each of
    the eight residue classes of the exponents gives G_m, and f(z0 u^j) = sum_m G_m (z0 u^j)^m - N products for eight values"""
    big = pow(z0, 8, R)
    g = []
    for m in range(8):
        acc = 0
        for c in reversed(coeffs[m::8]):
            acc = (acc * big + c) % R
        g.append(acc)
    u = pm.root_of_unity(3)
    zs = [z0 * pow(u, j, R) % R for j in range(8)]
    return zs, [sum(g[m] * pow(z, m, R) for m in range(8)) % R for z in zs]


@pytest.mark.parametrize("log2_n", [16, 20])
def test_ntt_large_dense_agrees_with_fr_eval_and_horner(eng, log2_n):
    """dense random coefficients c: fr_eval of ntt(c) at eight points outside the domain is Horner of c there"""
    rng = random.Random(0xE7A + log2_n)
    n = 1 << log2_n
    x = _dense(n, 100 + log2_n)
    raw = x.tobytes()
    coeffs = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]
    zs, want = horner8(coeffs, rng.randrange(2, R))
    assert len(set(zs)) == 8 and all(pow(z, n, R) != 1 for z in zs)
    if log2_n == 16:                                    # the grouped run against the plain one, where that is cheap
        for z, w in zip(zs, want):
            acc = 0
            for c in reversed(coeffs):
                acc = (acc * z + c) % R
            assert acc == w
    for bitrev in (True, False):
        ev = eng.fr_ntt(to_dev(x), log2_n, bitrev=bitrev)
        many = ev.reshape(1, n, 4).expand(8, n, 4).contiguous()
        got = eng.fr_eval(many.reshape(-1, 4), to_dev(fr_rows(zs)), log2_n, bitrev)
        assert got.cpu().numpy().tobytes() == fr_rows(want).tobytes(), (log2_n, bitrev)
        del many, ev


@pytest.mark.parametrize("log2_n", [0, 3, 10, 12])
def test_the_two_bit_reversal_conventions_are_one(eng, log2_n):
    """fr_eval(ntt(c, BITREV), z, bitrev=True) is Horner of c at z"""
    rng = random.Random(0xB17 + log2_n)
    n = 1 << log2_n
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    dom = pm.domain(log2_n)
    zs = [rng.randrange(R), 0, dom[n // 3]]
    want = [sum(c * pow(z, k, R) for k, c in enumerate(p)) % R for p, z in zip(polys, zs)]
    for bitrev in (True, False):
        ev = eng.fr_ntt(fr_rows([v for p in polys for v in p]), log2_n, bitrev=bitrev)
        assert eng.fr_eval(ev, fr_rows(zs), log2_n, bitrev).tobytes() == fr_rows(want).tobytes(), (log2_n, bitrev)


def test_one_context_with_a_growing_domain_table():
    """log2_n = 4, 12, 4, 13, 12 on a fresh context: the table grows between calls and the smaller sizes read it with a new stride"""
    from zkvm_pairings_amd import PairingEngine
    rng = random.Random(0x6120)
    e = PairingEngine(0)
    try:
        for log2_n in (4, 12, 4, 13, 12):
            for flags in (0, pm.INVERSE | pm.BITREV | pm.COSET):
                p = [rng.randrange(R) for _ in range(1 << log2_n)]
                assert e.fr_ntt(fr_rows(p), log2_n, **kw(flags)).tobytes() == fr_rows(pm.ntt_flags(p, log2_n, flags)).tobytes(), (log2_n, flags)
    finally:
        e.close()


def test_validation_mode_reports_r_in_the_last_element():
    from zkvm_pairings_amd import PairingEngine, ZkpError
    rng = random.Random(0x7A1)
    e = PairingEngine(0, validate=True)
    try:
        for log2_n, n_poly in ((0, 1), (5, 3), (11, 2)):
            n = n_poly << log2_n
            clean = fr_rows([rng.randrange(R) for _ in range(n - 1)] + [R - 1])
            want = fr_rows([v for j in range(n_poly) for v in
                            pm.ntt([int.from_bytes(clean[i].tobytes(), "little") for i in range(j << log2_n, (j + 1) << log2_n)], log2_n)])
            assert e.fr_ntt(clean, log2_n).tobytes() == want.tobytes()
            assert e.fr_ntt(to_dev(clean), log2_n).cpu().numpy().tobytes() == want.tobytes()
            assert e.take_validation_status() is False
            bad = clean.copy()
            bad[n - 1] = fr_rows([R])[0]
            with pytest.raises(ZkpError) as ei:
                e.fr_ntt(bad, log2_n)
            assert ei.value.status == -4
            e.fr_ntt(to_dev(bad), log2_n)
            assert e.take_validation_status() is True and e.take_validation_status() is False
    finally:
        e.close()


def test_argument_errors_are_refused(eng):
    from zkvm_pairings_amd import _lib
    lib, h = eng._lib, eng._h
    buf = np.zeros((4, 4), dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert lib.zkp_fr_ntt_batch(h, p, 1, 21, 0, p) == -1
    assert lib.zkp_fr_ntt_batch(h, p, 1, 2, 8, p) == -1 and lib.zkp_fr_ntt_batch(h, p, 1, 2, -1, p) == -1
    assert lib.zkp_fr_ntt_batch(h, p, (1 << 26) + 1, 0, 0, p) == -1 and lib.zkp_fr_ntt_batch(h, p, 65, 20, 0, p) == -1
    assert lib.zkp_fr_ntt_batch(h, None, 1, 2, 0, p) == -1 and lib.zkp_fr_ntt_batch(h, p, 1, 2, 0, None) == -1
    assert lib.zkp_fr_ntt_batch(None, p, 1, 2, 0, p) == -1
    assert lib.zkp_fr_ntt_batch_dev(h, None, 1, 2, 0, None, None) == -1 and lib.zkp_fr_ntt_batch_dev(h, p, 1, 21, 0, p, None) == -1
    assert lib.zkp_fr_ntt_batch(h, None, 0, 20, 7, None) == 0 and lib.zkp_fr_ntt_batch_dev(h, None, 0, 3, 0, None, None) == 0
    assert _lib.NTT_INVERSE == 1 and _lib.NTT_BITREV == 2 and _lib.NTT_COSET == 4
    with pytest.raises(ValueError):
        eng.fr_ntt(np.zeros((3, 4), dtype=np.uint64), 1)
    # log2_n = 0 is the identity, whatever the flags
    x = fr_rows([5, R - 1, 0])
    for flags in FLAGS:
        assert eng.fr_ntt(x, 0, **kw(flags)).tobytes() == x.tobytes()
    # Fr.ntt: the class-level name
    import zkvm_pairings_amd as z
    c = [1, 2, 3, R - 4]
    assert [int(v) for v in z.Fr.ntt(c, engine=eng)] == pm.ntt(c, 2)
    assert [int(v) for v in z.Fr.ntt(pm.ntt(c, 2, bitrev=True, coset=True), inverse=True, bitrev=True, coset=True, engine=eng)] == c
