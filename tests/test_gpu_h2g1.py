"""Hash-to-G1 on one MI355X through the C ABI (run with -m gpu): hash_to_field, the map, the cofactor and their composition against
tests/h2g1_model.py (Python integers and hashlib), byte for byte, host and _dev flavour byte-identical."""
import json
import os
import random

import numpy as np
import pytest

import h2g1_adversarial as ha
import h2g1_model as g
import minsig_pools as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = g.P
LENGTHS = (0, 1, 8, 9, 16, 17, 55, 56, 63, 64, 65, 119, 120, 1000)          # both sides of every padding boundary of b_0 (43-byte DST)


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def both(eng, name, arrays, **kw):
    """the engine method on host arrays and on resident tensors: the outputs must be the same bytes; returns the host ones"""
    import torch
    out_h = getattr(eng, name)(*arrays, **kw)
    out_d = getattr(eng, name)(*[dev(a) if isinstance(a, np.ndarray) else a for a in arrays],
                               **{k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    hs = out_h if isinstance(out_h, tuple) else (out_h,)
    ds = out_d if isinstance(out_d, tuple) else (out_d,)
    for a, b in zip(hs, ds):
        assert np.asarray(a).tobytes() == host(b).tobytes(), name
    return out_h


def wire(points):
    rows = [g.g1_words(p) for p in points]
    return np.array([r[0] for r in rows], dtype=np.uint64).reshape(-1, 12), np.array([r[1] for r in rows], dtype=np.uint8)


def seeded_msg(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


_MODEL = {}


def model_hash(msg, dst):
    """the model's point of a message, computed once per (message, tag)"""
    key = (msg, dst)
    if key not in _MODEL:
        _MODEL[key] = g.hash_to_g1(msg, dst)
    return _MODEL[key]


def test_rfc_vectors_and_their_field_elements(eng):
    with open(os.path.join(ROOT, "tests", "golden", "h2c_g1_vectors.json")) as f:
        kat = json.load(f)
    dst = kat["dst"].encode()
    msgs = [v["msg"].encode() for v in kat["vectors"]]
    pts, inf = eng.hash_to_g1(msgs, dst)
    want, winf = wire([tuple(int(c, 16) for c in v["p"]) for v in kat["vectors"]])
    assert pts.tobytes() == want.tobytes() and inf.tobytes() == winf.tobytes()
    u = eng.hash_to_field_g1([b""], dst)
    assert [g.words_fp(u[0, 0:6]), g.words_fp(u[0, 6:12])] == [int(x, 16) for x in kat["u_empty"]]


@pytest.mark.parametrize("dst", [g.QUICKNET_DST, g.RFC_DST], ids=["quicknet", "rfc"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_hash_to_g1_on_messages_of_every_length(eng, dst, n):
    """a short last wavefront, more than one workgroup of the map, every padding boundary of b_0; host arrays and resident tensors"""
    rng = random.Random(0xA1)
    pool = [seeded_msg(rng, k) for k in LENGTHS]
    msgs = [pool[(5 * i + n) % len(pool)] for i in range(n)]
    buf, off = eng.pack_messages(msgs)
    pts, inf = both(eng, "hash_to_g1", (buf, dst), offsets=off)
    want, winf = wire([model_hash(x, dst) for x in msgs])
    assert pts.tobytes() == want.tobytes() and inf.tobytes() == winf.tobytes()
    u = both(eng, "hash_to_field_g1", (buf, dst), offsets=off)
    assert u.tobytes() == b"".join(v.to_bytes(48, "little") for x in msgs for v in g.hash_to_field_g1(x, dst))
    again, ainf = both(eng, "g1_map_from_fields", (u,))
    assert again.tobytes() == pts.tobytes() and ainf.tobytes() == inf.tobytes()


def test_map_from_fields_on_adversarial_u(eng):
    """u = 0, +-sqrt(-1 / 11), the sixteen u on a pole of the isogeny (both branches), a doubling, a cancellation, both branches, p - 1"""
    cases = ha.field_cases()
    assert len(ha.pole_u()) == 16 and {sq for _, sq in ha.pole_u()} == {True, False}
    u = np.array([g.fp_words(c[1]) + g.fp_words(c[2]) for c in cases], dtype=np.uint64)
    pts, inf = both(eng, "g1_map_from_fields", (u,))
    model = [g.map_from_fields(c[1], c[2]) for c in cases]
    want, winf = wire(model)
    names = [c[0] for c in cases]
    assert model[names.index("cancel")] is None and model[names.index("pole_pole")] is None and model[names.index("doubling")] is not None
    for i, name in enumerate(names):
        assert pts[i].tobytes() == want[i].tobytes() and inf[i] == winf[i], name
    assert not np.asarray(eng.g1_is_valid(pts, inf))[inf == 0].any()


def test_clear_cofactor_on_small_orders_the_identity_and_points_outside_g1(eng):
    cases = ha.point_cases()
    pin, iin = wire([c[1] for c in cases])
    pts, inf = both(eng, "g1_clear_cofactor", (pin,), inf=iin)
    model = [g.clear_cofactor(c[1]) for c in cases]
    want, winf = wire(model)
    for i, c in enumerate(cases):
        assert pts[i].tobytes() == want[i].tobytes() and inf[i] == winf[i], c[0]
    by = dict(zip([c[0] for c in cases], model))
    assert by["order3_plus"] is None and by["order3_minus"] is None and by["identity"] is None and by["order11"] is None
    assert by["order3_plus_g1"] == by["g1_random"] and all(g.in_g1(p) for p in model)
    assert not np.asarray(eng.g1_is_valid(pts, inf))[inf == 0].any()
    none, _ = both(eng, "g1_clear_cofactor", (pin,))                                  # no infinity bytes: the identity's (0, 1) is then a point off the curve
    keep = iin == 0
    assert none[keep].tobytes() == pts[keep].tobytes()


def border_lanes(n, last):
    """where k_g1h_affine's shared inversion (one per wavefront of 64, prefix and suffix products through LDS) meets identities: lanes 0, 63
    and 64, where they exist; point n - 1, which every dead lane of a short wavefront reads again, when `last`; and at n = 130 the whole
    first wavefront, whose shared product is then 1, beside a live second one"""
    lanes = {j for j in (0, 63, 64) if j < n} | (set(range(64)) if n == 130 else set())
    lanes.discard(n - 1)
    if last:
        lanes.add(n - 1)
    return sorted(lanes)


BORDER_SIZES = [1, 64, 65, 127, 130]


@pytest.mark.parametrize("n", BORDER_SIZES)
def test_clear_cofactor_identities_at_the_borders_of_the_shared_inversion(eng, n):
    """a zero Z let into the product of a wavefront would zero its 63 neighbours: identities of all three kinds in turn - a flagged one,
    (0, +-2) of order 3, the point of order 11 - at the borders, every other row a point with a finite image"""
    by = dict(ha.point_cases())
    kinds = [by[k] for k in ("identity", "order3_plus", "order11", "order3_minus")]
    finite = [(k, q) for k, q in ha.point_cases() if _clear(q) is not None]
    assert len(finite) == 12 and all(_clear(q) is None for q in kinds)
    for last in ((True, False) if n in (65, 127) else (True,)):
        lanes = border_lanes(n, last)
        assert (n - 1 in lanes) == last and (n < 130 or lanes[:64] == list(range(64)))
        pts = [finite[(5 * j + n) % len(finite)][1] for j in range(n)]
        for k, j in enumerate(lanes):
            pts[j] = kinds[(k + n + last) % len(kinds)]
        pin, iin = wire(pts)
        got, inf = both(eng, "g1_clear_cofactor", (pin,), inf=iin)
        want, winf = wire([_clear(q) for q in pts])
        assert np.nonzero(winf)[0].tolist() == lanes
        for j in range(n):
            assert got[j].tobytes() == want[j].tobytes() and inf[j] == winf[j], (n, last, j)
        live = inf == 0
        assert not ((got[:, :6] == 0).all(axis=1) & (got[:, 6:] == 0).all(axis=1))[live].any()
        assert not np.asarray(eng.g1_is_valid(got, inf))[live].any()


_CLEARED = {}
_MAPPED = {}


def _clear(q):
    if q not in _CLEARED:
        _CLEARED[q] = g.clear_cofactor(q)
    return _CLEARED[q]


@pytest.mark.parametrize("n", [65, 130])
def test_map_from_fields_cancelling_pairs_at_the_borders_of_the_shared_inversion(eng, n):
    """the same placement through the map: (u, -u) gives Q + (-Q), the identity out of k_g1h_clear<false>'s sum, at lanes 0, 63, 64 and
    n - 1, at 130 in every lane of the first wavefront"""
    rng = random.Random(0xB0)
    us = [(rng.randrange(1, P), rng.randrange(1, P)) for _ in range(4)]
    lanes = border_lanes(n, True)
    pairs = [us[(3 * j + n) % len(us)] for j in range(n)]
    for j in lanes:
        pairs[j] = (pairs[j][0], P - pairs[j][0])
    u = np.array([g.fp_words(a) + g.fp_words(b) for a, b in pairs], dtype=np.uint64)
    got, inf = both(eng, "g1_map_from_fields", (u,))
    for a, b in pairs:
        if (a, b) not in _MAPPED:
            _MAPPED[(a, b)] = g.map_from_fields(a, b)
    want, winf = wire([_MAPPED[x] for x in pairs])
    assert np.nonzero(winf)[0].tolist() == lanes
    for j in range(n):
        assert got[j].tobytes() == want[j].tobytes() and inf[j] == winf[j], (n, j)
    live = inf == 0
    assert not ((got[:, :6] == 0).all(axis=1) & (got[:, 6:] == 0).all(axis=1))[live].any()
    assert not np.asarray(eng.g1_is_valid(got, inf))[live].any()


def test_one_call_over_the_slice_boundary(eng):
    """2^17 + 61 messages from a pool of 64, a first offset that is not zero: every row equals the model's point of its message"""
    import torch
    idx = mp.index_sequence()
    buf, off = mp.packed(idx)
    dst = g.QUICKNET_DST
    pts, inf = eng.hash_to_g1(dev(buf), dst, offsets=dev(off))
    torch.cuda.synchronize()
    pts, inf = host(pts), host(inf)
    want, winf = wire([model_hash(x, dst) for x in mp.pool_messages()])
    assert len(set(idx[mp.SLICE - 64:mp.SLICE].tolist())) > 8 and len(set(idx[mp.SLICE:].tolist())) > 8
    assert pts.tobytes() == want[idx].tobytes() and inf.tobytes() == winf[idx].tobytes()


def test_argument_errors(eng):
    from zkvm_pairings_amd import ZkpError
    with pytest.raises(ZkpError):
        eng.hash_to_g1([b"x"], b"")
    with pytest.raises(ZkpError):
        eng.hash_to_g1([b"x"], b"d" * 256)
    with pytest.raises(ZkpError):
        eng.hash_to_g1(np.zeros(4, dtype=np.uint8), b"tag", offsets=np.array([0, 3, 2], dtype=np.uint64))
    pts, inf = eng.hash_to_g1([], b"tag")
    assert pts.shape == (0, 12) and inf.shape == (0,)
