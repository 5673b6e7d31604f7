"""Compressed points on one MI355X (run with -m gpu): the square-root hooks against the CPU oracle, decompression of every class of
configs.raw_points_compressed against the model / construction, compression round trips, the resident-tensor flavours, and the
compressed points check against the uncompressed one.  Expected values come from the oracle (tests/oracle_lib.py), the Python
model (tests/compressed_model.py) or the construction of the inputs - never from the library under test."""
import random

import numpy as np
import pytest

import bls12_381_model as m
import compressed_model as cm
import oracle_lib as o

pytestmark = pytest.mark.gpu
P = m.P

G1_KAT = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
G2_KAT = bytes.fromhex("93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                       "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def _ints(vals, n=6):
    return np.array([o.to_limbs(v, n) for v in vals], dtype=np.uint64).reshape(len(vals), n)


def _expect_classes(cls, which_col):
    from zkvm_pairings_amd import configs
    return np.array([configs.COMPRESSED_EXPECT[c][which_col] for c in configs.COMPRESSED_CLASSES], dtype=np.uint8)[cls]


def test_fp_sqrt_matches_the_oracle(eng, ref_kats):
    rng = random.Random(0x51)
    k = ref_kats["fp_sqrt"]
    vals = [rng.randrange(P) for _ in range(4096)] + [0, 1, P - 1, k["input"], k["non_residue"]]
    vals += [v * v % P for v in vals[:512]]
    a = _ints(vals)
    out, sq = eng.fp_sqrt(a)
    for i, v in enumerate(vals):
        want = o.fp_sqrt(a[i])
        assert bool(sq[i]) == (want is not None), v
        assert np.array_equal(out[i], want if want is not None else np.zeros(6, dtype=np.uint64)), v
    assert o.from_limbs(out[4096 + 3]) == int(k["expected_debug"], 16)
    assert not sq[4096 + 2] and not sq[4096 + 4] and sq[4096] and sq[4096 + 1]
    assert sq.sum() > 2000 and (1 - sq).sum() > 1500


def test_fp2_sqrt_is_the_references_root(eng):
    rng = random.Random(0x52)
    vals = []
    for i in range(3072):
        a = (rng.randrange(P), rng.randrange(P))
        vals.append(m.f2_sqr(a) if i % 2 == 0 else a)                 # squares, and random elements (about half non-squares)
    vals += [(0, 0), (1, 0), (4, 0), (P - 1, 0), (P - 4, 0), (3, 0), (0, 1), (0, P - 1)]
    vals += [(rng.randrange(P), 0) for _ in range(64)]                  # a1 = 0, a0 square or not: the alpha == -1 branch
    a = np.array([np.concatenate([o.to_limbs(c0), o.to_limbs(c1)]) for c0, c1 in vals], dtype=np.uint64)
    out, sq = eng.fp2_sqrt(a)
    branches = 0
    for i in range(len(vals)):
        want = o.fp2_sqrt(a[i])
        assert bool(sq[i]) == (want is not None), vals[i]
        assert np.array_equal(out[i], want if want is not None else np.zeros(12, dtype=np.uint64)), vals[i]
        if want is not None and vals[i][1] == 0 and vals[i][0] and pow(vals[i][0], (P - 1) // 2, P) != 1:
            branches += 1
    assert branches >= 10
    assert (1 - sq[:3072]).sum() > 600


@pytest.mark.parametrize("which", [1, 2])
def test_decompress_every_class(eng, which):
    from zkvm_pairings_amd import configs
    n = 20000
    raw, cls, pts = configs.raw_points_compressed(eng, n, which, 0xD0 + which)
    got, inf, st = eng.decompress_points(raw, which)
    assert np.array_equal(st, _expect_classes(cls, 0))
    assert np.array_equal(inf, _expect_classes(cls, 1))
    known = np.isin(cls, (0, 1, 4))                                  # a curve point behind the string: decoded exactly (the subgroup
    assert np.array_equal(got[known], pts[known])                   # is not checked: wrong_subgroup decodes with status 0)
    assert not got[st != 0].any()
    ident = np.flatnonzero(inf == 1)
    assert ident.size and (got[ident, 6 * which] == 1).all()
    # a sample of every class against the model
    model_dec = cm.g1_decompress if which == 1 else cm.g2_decompress
    for c in range(len(configs.COMPRESSED_CLASSES)):
        for i in np.flatnonzero(cls == c)[:24]:
            s, pt = model_dec(raw[i].tobytes())
            assert s == st[i], (configs.COMPRESSED_CLASSES[c], i)
            if s == 0 and pt is not None:
                flat = [pt[0], pt[1]] if which == 1 else [pt[0][0], pt[0][1], pt[1][0], pt[1][1]]
                assert np.array_equal(got[i], np.concatenate([o.to_limbs(v) for v in flat]).astype(np.uint64))
    # validity of what decoded: the subgroup points pass, the others fail is_valid's subgroup test
    val = (eng.g1_is_valid if which == 1 else eng.g2_is_valid)(got, inf)
    assert (val[np.isin(cls, (0, 1, 5))] == 0).all() and (val[cls == 4] == 2).all()


@pytest.mark.parametrize("which", [1, 2])
def test_compress_round_trip_2p16(eng, which):
    from zkvm_pairings_amd import configs, synthetic
    n = 1 << 16
    gen = synthetic.G1_GENERATOR if which == 1 else synthetic.G2_GENERATOR
    pts, pinf = (eng.g1_mul if which == 1 else eng.g2_mul)(gen, synthetic.scalars(0xC0 + which, n))
    assert not pinf.any()
    inf = np.zeros(n, dtype=np.uint8)
    inf[::997] = 1
    raw = np.frombuffer(eng.compress_points(pts, which, inf), dtype=np.uint8).reshape(n, 48 * which)
    assert np.array_equal(raw, configs.compress_np(pts, which, inf))
    comp = cm.g1_compress if which == 1 else cm.g2_compress
    for i in list(range(0, n, 4099)) + [0, 997]:
        if inf[i]:
            want = comp(None)
        elif which == 1:
            want = comp((o.from_limbs(pts[i, :6]), o.from_limbs(pts[i, 6:])))
        else:
            want = comp(((o.from_limbs(pts[i, :6]), o.from_limbs(pts[i, 6:12])), (o.from_limbs(pts[i, 12:18]), o.from_limbs(pts[i, 18:]))))
        assert raw[i].tobytes() == want, i
    back, binf, bst = eng.decompress_points(raw, which)
    assert not bst.any() and np.array_equal(binf, inf)
    fin = inf == 0
    assert np.array_equal(back[fin], pts[fin])
    un, uinf, ust = eng.decode_points(eng.encode_points(pts, which, inf), which)
    assert not ust.any() and np.array_equal(un, back) and np.array_equal(uinf, binf)
    # the generator known answers, byte for byte
    g = synthetic.G1_GENERATOR if which == 1 else synthetic.G2_GENERATOR
    kat = G1_KAT if which == 1 else G2_KAT
    assert eng.compress_points(g, which) == kat
    gp, gi, gs = eng.decompress_points(kat, which)
    assert gs[0] == 0 and gi[0] == 0 and np.array_equal(gp[0], np.asarray(g, dtype=np.uint64).reshape(-1))


def test_dev_flavours_equal_the_host_flavours(eng):
    import torch
    from zkvm_pairings_amd import configs
    for which in (1, 2):
        raw, cls, _ = configs.raw_points_compressed(eng, 3000, which, 4321 + which)
        pts, inf, st = eng.decompress_points(raw, which)
        t = torch.from_numpy(raw).cuda()
        dp, di, ds = eng.decompress_points_dev(t, which)
        assert np.array_equal(dp.cpu().numpy().view(np.uint64), pts) and np.array_equal(di.cpu().numpy(), inf) and np.array_equal(ds.cpu().numpy(), st)
        pad = torch.empty(raw.size + 3, dtype=torch.uint8, device="cuda")       # an unaligned view: the byte-wise kernel
        pad[3:] = t.reshape(-1)
        up, ui, us = eng.decompress_points_dev(pad[3:], which)
        assert torch.equal(up, dp) and torch.equal(ui, di) and torch.equal(us, ds)
        good = np.flatnonzero(st == 0)
        gi = torch.from_numpy(good).cuda()
        enc = eng.compress_points_dev(dp[gi].contiguous(), which, di[gi].contiguous())
        host = eng.compress_points(pts[good], which, inf[good])
        assert enc.cpu().numpy().tobytes() == host
        # compressing into an unaligned output: the byte-wise store path, same bytes
        n = good.size
        out = torch.empty(n * 48 * which + 5, dtype=torch.uint8, device="cuda")
        rc = eng._lib.zkp_g1_compress_batch_dev if which == 1 else eng._lib.zkp_g2_compress_batch_dev
        eng._chk(rc(eng._h, eng._tp(dp[gi].contiguous()), eng._tp(di[gi].contiguous()), n, eng._tp(out[5:]), eng._stream()))
        torch.cuda.synchronize()
        assert out[5:].cpu().numpy().tobytes() == host


def _uncompressed_twin(raw, cls, pts, which):
    """the uncompressed encoding of the same inputs: the same point where there is one, and strings that fail the uncompressed
    decode / is_valid with the same status where there is none"""
    from zkvm_pairings_amd import configs
    w = 96 * which
    un = configs.to_bytes(pts, which).copy()
    nc = np.flatnonzero(cls == 2)
    un[nc, :48] = raw[nc, :48]
    un[nc, 0] &= 0x1F                                               # same x >= p, no flag
    off = np.flatnonzero(cls == 3)
    un[off] = 0
    un[off, :48 * which] = raw[off]
    un[off, 0] &= 0x1F                                              # (x, 0): decodes, then fails is_valid's curve test
    un[cls == 5] = 0
    un[cls == 5, 0] = 0x40
    un[cls == 6, 0] |= 0x40
    un[cls == 7, 0] |= 0x80
    assert un.shape[1] == w
    return un


def test_compressed_points_check_against_the_oracle_and_the_uncompressed_check(eng):
    from zkvm_pairings_amd import configs
    n = 600
    r1, c1, p1 = configs.raw_points_compressed(eng, n, 1, 0xA1)
    r2, c2, p2 = configs.raw_points_compressed(eng, n, 2, 0xA2)
    # every class in either position
    perm = np.random.default_rng(3).permutation(n)
    r2, c2, p2 = r2[perm], c2[perm], p2[perm]
    u1, u2 = _uncompressed_twin(r1, c1, p1, 1), _uncompressed_twin(r2, c2, p2, 2)
    e1, e2 = _expect_classes(c1, 2), _expect_classes(c2, 2)
    for k in (1, 3):
        s1, s2, ok, allok = eng.points_check_compressed(r1, r2, k)
        assert np.array_equal(s1, e1) and np.array_equal(s2, e2)
        us1, us2, uok, uallok = eng.points_check(u1, u2, k)
        assert np.array_equal(s1, us1) and np.array_equal(s2, us2) and np.array_equal(ok, uok) and allok == uallok
        # ok against the oracle: every point of the check valid and the product of its pairings the identity
        valid = ((e1 == 0) & (e2 == 0)).reshape(-1, k).all(axis=1)
        inf1 = (c1 == 5).astype(np.uint8)
        inf2 = (c2 == 5).astype(np.uint8)
        idx = np.flatnonzero(valid)
        sel = (idx[:, None] * k + np.arange(k)[None, :]).reshape(-1)
        want = np.zeros(n // k, dtype=np.uint8)
        if idx.size:
            okv = o.pairing_check_batch(p1[sel], p2[sel], idx.size, k, inf1[sel], inf2[sel])
            want[idx] = okv
        assert np.array_equal(ok, want), k
        assert allok == bool(want.all())


def test_config5_compressed_at_2p20_equals_the_uncompressed_check(eng):
    """config 5 in compressed form at 2^20 pairs: status bytes, ok bytes and the AND flag equal those of points_check on the
    uncompressed encoding of the same points; checks are (P, Q), (-P, Q) pairs so that valid checks pass"""
    from zkvm_pairings_amd import configs
    n = 1 << 19
    r1, c1, p1 = configs.raw_points_compressed(eng, n, 1, 0x5EED1)
    r2, c2, p2 = configs.raw_points_compressed(eng, n, 2, 0x5EED2)
    u1, u2 = _uncompressed_twin(r1, c1, p1, 1), _uncompressed_twin(r2, c2, p2, 2)
    # pair j: (P_j, Q_j) and (-P_j, Q_j)
    neg_r1 = r1.copy()
    flip = np.isin(c1, (0, 1, 4))
    neg_r1[flip, 0] ^= 0x20
    neg_p1 = configs.negate_g1(eng, p1)
    neg_u1 = u1.copy()
    neg_u1[flip] = configs.to_bytes(neg_p1[flip], 1)
    inter = lambda a, b: np.stack([a, b], axis=1).reshape(2 * a.shape[0], -1)
    b1c, b2c = inter(r1, neg_r1), inter(r2, r2)
    b1u, b2u = inter(u1, neg_u1), inter(u2, u2)
    s1, s2, ok, allok = eng.points_check_compressed(b1c, b2c, 2)
    us1, us2, uok, uallok = eng.points_check(b1u, b2u, 2)
    assert np.array_equal(s1, us1) and np.array_equal(s2, us2)
    assert np.array_equal(ok, uok) and allok == uallok
    e1, e2 = _expect_classes(c1, 2), _expect_classes(c2, 2)
    assert np.array_equal(s1[0::2], e1) and np.array_equal(s2[0::2], e2)
    assert np.array_equal(ok, ((e1 == 0) & (e2 == 0)).astype(np.uint8))      # e(P,Q) e(-P,Q) == 1 for every valid pair
    assert not allok and ok.sum() > n // 2


def test_compressed_points_check_is_capturable(eng):
    import torch
    from zkvm_pairings_amd import synthetic
    dev = torch.device("cuda", 0)
    n = 4096
    g1, g2, _, _ = synthetic.random_pairs(eng, n, seed=78, device_tensors=True)
    b1, b2 = eng.compress_points_dev(g1, 1), eng.compress_points_dev(g2, 2)
    b1[3::5, 47] ^= 1                                                 # another x: off the curve or outside the subgroup
    st1 = torch.empty(n, dtype=torch.uint8, device=dev)
    st2 = torch.empty_like(st1)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    eng.points_check_compressed(b1, b2, 1, st1, st2, ok, flag)
    torch.cuda.synchronize()
    want = (st1.clone(), st2.clone(), ok.clone(), flag.clone())
    assert (want[0][3::5] != 0).all() and int((want[0] != 0).sum()) == len(range(3, n, 5))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.points_check_compressed(b1, b2, 1, st1, st2, ok, flag)
    for t in (st1, st2, ok):
        t.fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, (st1, st2, ok, flag)))
    b1[3::5, 47] ^= 1
    graph.replay()
    torch.cuda.synchronize()
    assert not st1.any() and not st2.any() and int(flag.item()) == 0 and not ok.any()
    eng.points_check_compressed(b1, b2, 1, st1, st2, ok, flag)
    torch.cuda.synchronize()
    assert not st1.any() and int(flag.item()) == 0


def test_bad_arguments(eng):
    from zkvm_pairings_amd import PairingEngine, _lib
    lib, h = eng._lib, eng._h
    ERR_ARG = -1
    assert lib.zkp_fp_sqrt_batch(h, None, 1, None, None) == ERR_ARG
    assert lib.zkp_fp2_sqrt_batch(None, None, 0, None, None) == ERR_ARG
    assert lib.zkp_g1_decompress_batch(h, None, 1, None, None, None) == ERR_ARG
    assert lib.zkp_g2_compress_batch(h, None, None, 1, None) == ERR_ARG
    assert lib.zkp_g1_decompress_batch_dev(h, None, 1, None, None, None, None) == ERR_ARG
    assert lib.zkp_g2_compress_batch_dev(None, None, None, 0, None, None) == ERR_ARG
    assert lib.zkp_points_check_compressed_batch(h, None, None, 1, 1, None, None, None, None) == ERR_ARG
    assert lib.zkp_points_check_compressed_batch_dev(h, None, None, 1, 1, None, None, None, None, None) == ERR_ARG
    assert lib.zkp_points_check_compressed_batch(h, None, None, 1 << 31, 1, None, None, None, None) == ERR_ARG
    with pytest.raises(ValueError):
        eng.points_check_compressed(np.zeros((3, 48), dtype=np.uint8), np.zeros((2, 96), dtype=np.uint8), 1)
    with pytest.raises(ValueError):
        eng.decompress_points(bytes(47), 1)
    v = PairingEngine(0, validate=True)
    try:
        with pytest.raises(_lib.ZkpError) as ei:
            v.fp_sqrt(o.to_limbs(P))
        assert ei.value.status == -4
        with pytest.raises(_lib.ZkpError) as ei:
            v.fp2_sqrt(np.concatenate([o.to_limbs(1), o.to_limbs(P + 3)]))
        assert ei.value.status == -4
        out, sq = v.fp_sqrt(o.to_limbs(4))
        assert sq[0] == 1 and o.from_limbs(out[0]) in (2, P - 2)
    finally:
        v.close()


def test_affine_types_round_trip(eng):
    from zkvm_pairings_amd.pairings import G1Affine, G2Affine
    g1, g2 = G1Affine.generator(), G2Affine.generator()
    assert g1.to_compressed(eng) == G1_KAT and g2.to_compressed(eng) == G2_KAT
    assert G1Affine.from_compressed(G1_KAT, eng) == g1 and G2Affine.from_compressed(G2_KAT, eng) == g2
    assert G1Affine.from_compressed(G1Affine.identity().to_compressed(eng), eng).is_identity()
    with pytest.raises(ValueError):
        G1Affine.from_compressed(bytes([G1_KAT[0] & 0x7F]) + G1_KAT[1:], eng)
