"""Hash-to-G2 on one MI355X through the C ABI (run with -m gpu): the wide reduction, hash_to_field, the map, the cofactor and their
composition against tests/h2c_model.py (Python integers and hashlib), host and _dev flavour byte-identical."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

import bls12_381_model as m
import bls_replay_cases as brc
import h2c_model as h
import outside_groups as og

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = h.P
LENGTHS = (0, 1, 8, 9, 16, 17, 55, 56, 63, 64, 65, 119, 120, 1000)          # both sides of every padding boundary of b_0 (43-byte DST)
DST_LENGTHS = (1, 21, 22, 43, 85, 86, 255)                                   # b_i: one block becomes two at 22, two three at 86


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


def seeded_msg(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def test_fp_from_wide_be(eng):
    q = (1 << 512) // P
    vals = [0, 1, P - 1, P, P + 1, (1 << 384) - 1, 1 << 384, (1 << 512) - 1, q * P - 1, q * P, q * P + 1]
    vals += [1 << b for b in range(0, 512, 28)] + [(1 << b) - 1 for b in range(28, 512, 28)]
    vals += [1 << b for b in range(0, 512, 32)] + [(1 << b) - 1 for b in range(32, 512, 32)]
    rng = random.Random(0x51DE)
    vals += [rng.randrange(1 << 512) for _ in range(1024)]
    data = np.frombuffer(b"".join(v.to_bytes(64, "big") for v in vals), dtype=np.uint8).reshape(-1, 64)
    got = both(eng, "fp_from_wide_be", (data,))
    want = brc.u64([h.fp_words(v % P) for v in vals])
    assert got.tobytes() == want.tobytes()


def test_hash_to_field_mixed_lengths_in_one_call(eng):
    """lanes of one wavefront take different block counts"""
    rng = random.Random(1)
    msgs = [seeded_msg(rng, n) for n in LENGTHS] + [seeded_msg(rng, n) for n in (72, 73, 2, 31, 32, 33)]
    for dst_len in DST_LENGTHS:
        dst = h.ETH_DST if dst_len == 43 else seeded_msg(rng, dst_len)
        buf, off = brc.pack(msgs)
        got = both(eng, "hash_to_field_g2", (buf, dst), offsets=off)
        assert got.tobytes() == brc.field_rows(msgs, dst).tobytes(), dst_len
    one = both(eng, "hash_to_field_g2", brc.pack([b"abc"])[:1] + (h.RFC_DST,), offsets=brc.pack([b"abc"])[1])
    assert one.tobytes() == brc.field_rows([b"abc"], h.RFC_DST).tobytes()


@pytest.mark.parametrize("n", [65, 129])
@pytest.mark.parametrize("base", [1, 2, 3])
def test_hash_to_field_equal_messages_at_unaligned_offsets(eng, n, base):
    msg = bytes(range(37))
    buf, off = brc.pack([msg] * n, base=base)
    got = both(eng, "hash_to_field_g2", (buf, h.ETH_DST), offsets=off)
    want = brc.field_rows([msg], h.ETH_DST)
    assert got.tobytes() == np.repeat(want, n, axis=0).tobytes()


def _u_rows(us):
    return brc.u64([h.f2_words(a) + h.f2_words(b) for a, b in us]).reshape(-1, 24)


def test_map_from_fields_edge_cases_and_both_branches(eng):
    g = m.SplitMix64(0x5EED)
    rnd = lambda: (g.below(P), g.below(P))
    a = rnd()
    us = [((0, 0), (0, 0)), (a, a), (a, m.f2_neg(a)), ((0, 0), a)]
    us += [(s, rnd()) for s in ((0, 1), (0, 2), (1, 0), (2, 0), (P - 1, 0), (0, P - 1))]
    us += [(rnd(), rnd()) for _ in range(12)]
    assert {h.sswu(u)[1] for pair in us for u in pair} == {True, False}
    pts, inf = both(eng, "g2_map_from_fields", (_u_rows(us),))
    want, winf = brc.point_rows([h.map_from_fields(x, y) for x, y in us])
    assert winf[2] == 1 and inf.tobytes() == winf.tobytes()
    assert pts.tobytes() == want.tobytes()


def test_clear_cofactor(eng):
    g = m.SplitMix64(3)
    pts = [None, m.G2_GEN, m.g2_mul(m.G2_GEN, 12345)]
    pts += [h.iso3(h.sswu((g.below(P), g.below(P)))[0]) for _ in range(5)]
    fixtures = [q for q in og.g2_points().values() if m.g2_on_curve(q)]
    pts += fixtures
    rows, inf = brc.point_rows(pts)
    got, ginf = both(eng, "g2_clear_cofactor", (rows,), inf=inf)
    model = [h.clear_cofactor_psi(q) for q in pts]
    assert model[1] == m.g2_mul(m.G2_GEN, h.H_EFF % h.R_ORDER)
    assert any(q is None for q in model[8:]) or not fixtures                 # small-order fixtures go to the identity
    want, winf = brc.point_rows(model)
    assert ginf.tobytes() == winf.tobytes() and got.tobytes() == want.tobytes()
    assert not eng.g2_is_valid(got, ginf).any()


def test_map_from_fields_on_colliding_and_real_g_elements(eng):
    """tests/h2c_adversarial.py in one call: pairs of different u with one image or opposite images (k_h2c_clear's first addition meets
    H = 0, and r = 0 or not, on operands computed from different u, for the cross pairs along different branches of the map)
    and u whose g(x1) lies in Fp (a residue: the root is real; a non-residue: the fallback of f2_sqrt_with_norm, a purely imaginary root).
    tests/test_h2c_cpu.py has shown that the inputs are what they are called"""
    import h2c_adversarial as ha
    rows = ha.inputs()
    pts, inf = both(eng, "g2_map_from_fields", (_u_rows([(a, b) for _, a, b in rows]),))
    want, winf = brc.point_rows(ha.expected())
    assert winf.sum() == 8
    for j, (label, _, _) in enumerate(rows):
        assert inf[j] == winf[j] and pts[j].tobytes() == want[j].tobytes(), (j, label)
    assert not eng.g2_is_valid(pts, inf).any()


def test_clear_cofactor_through_every_reachable_addition_branch(eng):
    """the inputs whose additions tests/test_h2c_cpu.py has traced branch by branch (COFACTOR_BRANCHES there): the identity, points of G2,
    every multiple of a point of order 13, the other small orders, and their sums with a point of G2; and four multiples of the generator
    whose doubling at B = psi(P) - A meets an H that is zero mod p with non-zero limbs (NEAR_ZERO_MULTIPLES of tests/h2c_adversarial.py)"""
    import h2c_adversarial as ha
    cases = ha.cofactor_points()
    rows, inf = brc.point_rows([q for _, q in cases])
    got, ginf = both(eng, "g2_clear_cofactor", (rows,), inf=inf)
    want, winf = brc.point_rows([r for r, _ in ha.cofactor_traces()])
    assert 0 < winf.sum() < len(cases)
    for j, (label, _) in enumerate(cases):
        assert ginf[j] == winf[j] and got[j].tobytes() == want[j].tobytes(), (j, label)
    assert not eng.g2_is_valid(got, ginf).any()


def test_hash_to_g2_rfc_vectors_and_seeded_messages(eng):
    with open(os.path.join(ROOT, "tests", "golden", "h2c_vectors.json")) as f:
        v = json.load(f)
    msgs = [c["msg"].encode() for c in v["vectors"]]
    pts, inf = both(eng, "hash_to_g2", brc.pack(msgs)[:1] + (v["dst"].encode(),), offsets=brc.pack(msgs)[1])
    want = brc.u64([[w for x in c["p"] for w in h.fp_words(int(x, 16))] for c in v["vectors"]])
    assert not inf.any() and pts.tobytes() == want.tobytes()
    rng = random.Random(0x300)
    many = [seeded_msg(rng, rng.randrange(0, 201)) for _ in range(300)]
    buf, off = brc.pack(many)
    pts, inf = both(eng, "hash_to_g2", (buf, h.ETH_DST), offsets=off)
    want, winf = brc.point_rows([brc.hashed(x, h.ETH_DST) for x in many])
    assert inf.tobytes() == winf.tobytes() and pts.tobytes() == want.tobytes()
    assert not eng.g2_is_valid(pts, inf).any()
    # the list form of the package
    import zkvm_pairings_amd as z
    p2, _ = z.hash_to_g2(many[:5], h.ETH_DST, engine=eng)
    assert p2.tobytes() == want[:5].tobytes()


def test_argument_errors(eng):
    lib, hh = eng._lib, eng._h
    buf, off = brc.pack([b"abc", b""])
    out, oi = np.zeros((2, 24), dtype=np.uint64), np.zeros(2, dtype=np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    d = np.frombuffer(h.ETH_DST, dtype=np.uint8)
    assert lib.zkp_hash_to_g2_batch(hh, p(buf), p(off), 2, p(d), 0, p(out), p(oi)) == -1
    assert lib.zkp_hash_to_g2_batch(hh, p(buf), p(off), 2, p(d), 256, p(out), p(oi)) == -1
    assert lib.zkp_hash_to_g2_batch(hh, p(buf), None, 2, p(d), d.size, p(out), p(oi)) == -1
    assert lib.zkp_hash_to_g2_batch(hh, p(buf), p(off), 2, None, d.size, p(out), p(oi)) == -1
    assert lib.zkp_hash_to_g2_batch(hh, p(buf), p(off), 2, p(d), d.size, None, p(oi)) == -1
    assert lib.zkp_hash_to_g2_batch(hh, p(buf), p(off), 1 << 31, p(d), d.size, p(out), p(oi)) == -1
    assert lib.zkp_hash_to_field_g2_batch(hh, p(buf), p(off), 2, p(d), d.size, None) == -1
    assert lib.zkp_fp_from_wide_be_batch(hh, None, 1, p(out)) == -1
    assert lib.zkp_g2_map_from_fields_batch(hh, p(out), 1, p(out), None) == -1
    assert lib.zkp_g2_clear_cofactor_batch(hh, None, None, 1, p(out), p(oi)) == -1
    bad = off[::-1].copy()
    assert lib.zkp_hash_to_g2_batch(hh, p(buf), p(bad), 2, p(d), d.size, p(out), p(oi)) == -1          # the host flavour sees the offsets
    assert lib.zkp_hash_to_g2_batch(hh, p(buf), p(off), 0, p(d), d.size, None, None) == 0


def test_decreasing_offsets_hash_as_empty_and_raise_the_validation_word():
    import torch
    from zkvm_pairings_amd import PairingEngine
    msgs = [b"first", b"second message", b"third"]
    buf, off = brc.pack(msgs)
    bad = off.copy()
    bad[2] = bad[1] - 3                                                        # message 1 runs backwards, message 2 starts before message 1
    want = brc.field_rows([msgs[0], b"", b""], h.ETH_DST)
    want[2] = brc.field_rows([buf[int(bad[2]):int(bad[3])].tobytes()], h.ETH_DST)[0]   # message 2 is still a range inside the buffer
    for validate in (False, True):
        e = PairingEngine(0, validate=validate)
        try:
            got = e.hash_to_field_g2(dev(buf), h.ETH_DST, offsets=dev(bad))
            torch.cuda.synchronize()
            assert host(got).tobytes() == want.tobytes()
            word = ctypes.c_int(-1)
            assert e._lib.zkp_take_validation_status_dev(e._h, e._stream(), ctypes.byref(word)) == 0
            assert word.value == (1 if validate else 0)
            ok = e.hash_to_field_g2(dev(buf), h.ETH_DST, offsets=dev(off))
            torch.cuda.synchronize()
            assert host(ok).tobytes() == brc.field_rows(msgs, h.ETH_DST).tobytes()
        finally:
            e.close()


def test_c_consumer(tmp_path):
    libdir = os.path.join(ROOT, "zkvm_pairings_amd")
    exe = str(tmp_path / "zkp_bls")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "c", "zkp_bls.c"), "-L", libdir,
                           "-lzkp_pairings", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("zkp_bls ok"), (out.returncode, out.stdout, out.stderr)
