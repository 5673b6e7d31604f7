"""The two flavours of every entry point (run with -m gpu on an MI355X): a host-pointer call stages its inputs and runs the same
launch-only code as its *_dev twin, so on the same seeded inputs both give the same bytes and the same status, on either kernel
family.  In validation mode a non-canonical input fails the host flavour with ZKP_ERR_NONCANONICAL before any launch and sets the
sticky word of the *_dev flavour; a host call never touches that word."""
import numpy as np
import pytest

import bls12_381_model as m
import oracle_lib as o

pytestmark = pytest.mark.gpu

ERR_NONCANONICAL = -4


@pytest.fixture(scope="module", params=["thread", "coop"])
def eng(request):
    from zkvm_pairings_amd import PairingEngine, _lib
    e = PairingEngine(0)
    try:
        e.set_kernel(request.param)
    except _lib.ZkpError:
        e.close()
        pytest.skip("kernel family %s not available in this build" % request.param)
    yield e
    e.close()


def _t(a):
    """numpy array -> tensor on GPU 0 (uint64 as int64, the engine's convention)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def _same(host, dev):
    import torch
    torch.cuda.synchronize()
    d = dev.cpu().numpy()
    d = d.view(np.uint64) if d.dtype == np.int64 else d
    h = np.frombuffer(host, dtype=np.uint8) if isinstance(host, bytes) else np.asarray(host)
    assert h.dtype == d.dtype and np.array_equal(h.reshape(-1), d.reshape(-1))


def _inputs(eng):
    """16 checks of k = 2 pairs (aP, bQ), (-abP, Q): every third check broken; infinity flags on a few pairs"""
    from zkvm_pairings_amd import synthetic
    n = 16
    g1, g2, a, b = synthetic.random_pairs(eng, n, seed=0x5EED)
    ab = np.stack([synthetic.int_to_scalar((-synthetic.scalar_to_int(x) * synthetic.scalar_to_int(y)) % synthetic.R_ORDER) for x, y in zip(a, b)])
    p3, _ = eng.g1_mul(synthetic.G1_GENERATOR, ab)
    broken = np.arange(0, n, 3)
    p3[broken] = p3[(broken + 1) % n]
    G1 = np.ascontiguousarray(np.stack([g1, p3], axis=1).reshape(2 * n, 12))
    G2 = np.ascontiguousarray(np.stack([g2, np.tile(synthetic.G2_GENERATOR, (n, 1))], axis=1).reshape(2 * n, 24))
    inf1 = np.zeros(2 * n, dtype=np.uint8)
    inf1[[5, 12]] = 1
    inf2 = np.zeros(2 * n, dtype=np.uint8)
    inf2[[12, 21]] = 1
    return G1, G2, inf1, inf2, a


def test_host_flavours_equal_the_dev_flavours(eng):
    import torch
    from zkvm_pairings_amd import synthetic
    G1, G2, inf1, inf2, sc = _inputs(eng)
    t1, t2, ti1, ti2 = _t(G1), _t(G2), _t(inf1), _t(inf2)
    k = 2
    # pairing family
    _same(eng.pairing(G1, G2, inf1, inf2), eng.pairing(t1, t2, ti1, ti2))
    ml = eng.multi_miller_loop(G1, G2, k, inf1, inf2)
    _same(ml, eng.multi_miller_loop(t1, t2, k, ti1, ti2))
    _same(eng.final_exponentiation(ml), eng.final_exponentiation(_t(ml)))
    _same(eng.fp12_product(ml), eng.fp12_product(_t(ml)))
    _same(eng.miller_product(G1, G2, inf1, inf2), eng.miller_product(t1, t2, ti1, ti2))
    for lo, hi in ((2, 6), (0, len(G1))):                             # two good checks (the identity), then all sixteen
        gt, one = eng.pairing_product_check(G1[lo:hi], G2[lo:hi])
        dgt, done = eng.pairing_product_check(t1[lo:hi], t2[lo:hi])
        _same(gt, dgt)
        assert one == bool(done.item()) and one == (hi == 6)
    ok, allok = eng.pairing_check(G1, G2, k, inf1, inf2)
    dok, dallok = eng.pairing_check(t1, t2, k, ti1, ti2)
    _same(ok, dok)
    assert allok == bool(dallok.item()) and 0 < ok.sum() < len(ok)
    # is_valid: off the curve, and on it but outside the subgroup (the first x whose x^3 + 4 is a square; p = 3 mod 4)
    bad1, bad2 = G1[:8].copy(), G2[:8].copy()
    bad1[1, 6:] = o.to_limbs(1)
    bad2[2, 18:] = o.to_limbs(3)
    x = next(v for v in range(1, 100) if pow(v ** 3 + 4, (m.P - 1) // 2, m.P) == 1)
    bad1[3] = np.concatenate([o.to_limbs(x), o.to_limbs(pow(x ** 3 + 4, (m.P + 1) // 4, m.P))])
    vinf = np.array([0, 0, 0, 0, 1, 0, 0, 0], dtype=np.uint8)
    st = eng.g1_is_valid(bad1, vinf)
    _same(st, eng.g1_is_valid(_t(bad1), _t(vinf)))
    assert st[1] == 1 and st[3] == 2
    st = eng.g2_is_valid(bad2)
    _same(st, eng.g2_is_valid(_t(bad2)))
    assert st[2] == 1
    # scalar multiplication: one broadcast base, and a base per scalar; the zero scalar gives the identity
    s = sc.copy()
    s[3] = 0
    for which, base in ((1, synthetic.G1_GENERATOR), (2, synthetic.G2_GENERATOR), (1, G1[: len(s)]), (2, G2[: len(s)])):
        mul = eng.g1_mul if which == 1 else eng.g2_mul
        p, pi = mul(base, s)
        dp, dpi = mul(_t(base), _t(s))
        _same(p, dp)
        _same(pi, dpi)
        assert pi[3] == 1
    # addition with P + P, P + (-P) and infinity inputs
    for which, pts in ((1, G1), (2, G2)):
        cols = 12 * which
        a, b = pts[:8].copy(), pts[8:16].copy()
        b[0] = a[0]
        b[1, :cols // 2] = a[1, :cols // 2]
        b[1, cols // 2:] = np.concatenate([o.to_limbs((m.P - o.from_limbs(a[1, j:j + 6])) % m.P) for j in range(cols // 2, cols, 6)])
        ia, ib = np.zeros(8, dtype=np.uint8), np.zeros(8, dtype=np.uint8)
        ia[2], ib[3] = 1, 1
        add = eng.g1_add if which == 1 else eng.g2_add
        r, ri = add(a, b, ia, ib)
        dr, dri = add(_t(a), _t(b), _t(ia), _t(ib))
        _same(r, dr)
        _same(ri, dri)
        assert ri[1] == 1 and ri.sum() == 1
    # multi-scalar multiplication: three sums of eight terms, own and shared bases
    for which, pts in ((1, G1), (2, G2)):
        msm = eng.g1_msm if which == 1 else eng.g2_msm
        scal = np.ascontiguousarray(np.concatenate([sc, sc[::-1]])[:24])
        for shared, npts in ((False, 24), (True, 8)):
            pinf = np.zeros(npts, dtype=np.uint8)
            pinf[1] = 1
            r, ri = msm(pts[:npts], scal, 3, inf=pinf, shared_bases=shared)
            dr, dri = msm(_t(pts[:npts]), _t(scal), 3, inf=_t(pinf), shared_bases=shared)
            _same(r, dr)
            _same(ri, dri)
    # both codecs, well-formed and malformed strings, with and without infinity flags
    for which, pts in ((1, G1), (2, G2)):
        pinf = np.zeros(len(pts), dtype=np.uint8)
        pinf[7] = 1
        for fl in (None, pinf):
            raw = eng.encode_points(pts, which, fl)
            _same(raw, eng.encode_points_dev(_t(pts), which, None if fl is None else _t(fl)))
            cmp = eng.compress_points(pts, which, fl)
            _same(cmp, eng.compress_points_dev(_t(pts), which, None if fl is None else _t(fl)))
        raw = np.frombuffer(raw, dtype=np.uint8).reshape(len(pts), -1).copy()
        raw[0, :48] = np.frombuffer(m.P.to_bytes(48, "big"), dtype=np.uint8)   # a coordinate >= p
        raw[1, 0] |= 0x80                                                       # a compression flag
        for h, d in zip(eng.decode_points(raw, which), eng.decode_points_dev(_t(raw), which)):
            _same(h, d)
        cmp = np.frombuffer(cmp, dtype=np.uint8).reshape(len(pts), -1).copy()
        cmp[2, 0] &= 0x7F                                                       # no compression flag
        cmp[3, 1] ^= 0x55                                                       # most such x have no point
        for h, d in zip(eng.decompress_points(cmp, which), eng.decompress_points_dev(_t(cmp), which)):
            _same(h, d)
    # points checks, uncompressed and compressed, with a few broken points
    for compressed in (False, True):
        if compressed:
            b1, b2 = eng.compress_points(G1, 1), eng.compress_points(G2, 2)
        else:
            b1, b2 = eng.encode_points(G1, 1), eng.encode_points(G2, 2)
        b1 = np.frombuffer(b1, dtype=np.uint8).reshape(len(G1), -1).copy()
        b2 = np.frombuffer(b2, dtype=np.uint8).reshape(len(G2), -1).copy()
        b1[4, 0] ^= 0x80                                                        # the compression flag flipped: malformed
        b2[9, -1] ^= 1
        check = eng.points_check_compressed if compressed else eng.points_check
        s1, s2, okb, allok = check(b1, b2, k)
        d1, d2 = torch.empty(len(G1), dtype=torch.uint8, device="cuda"), torch.empty(len(G1), dtype=torch.uint8, device="cuda")
        dokb, dall = torch.empty(len(G1) // k, dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
        check(_t(b1), _t(b2), k, d1, d2, dokb, dall)
        for h, d in ((s1, d1), (s2, d2), (okb, dokb)):
            _same(h, d)
        assert allok == bool(dall.item()) and s1[4] and s2[9] and not okb[2] and okb.any()


def test_validation_mode_fails_the_host_flavour_and_flags_the_dev_flavour(eng):
    from zkvm_pairings_amd import _lib
    G1, G2, _, _, sc = _inputs(eng)
    ml = eng.multi_miller_loop(G1, G2, 2)
    P_LIMBS = o.to_limbs(m.P)
    b1, b2, bml = G1.copy(), G2.copy(), ml.copy()
    b1[3, :6] = P_LIMBS
    b2[6, 6:12] = P_LIMBS
    bml[1, 12:18] = P_LIMBS
    calls = [
        ("pairing g1", lambda g1, g2, f: eng.pairing(g1, g2), 0),
        ("pairing g2", lambda g1, g2, f: eng.pairing(g1, g2), 1),
        ("miller loop", lambda g1, g2, f: eng.multi_miller_loop(g1, g2, 2), 1),
        ("final exponentiation", lambda g1, g2, f: eng.final_exponentiation(f), 2),
        ("fp12 product", lambda g1, g2, f: eng.fp12_product(f), 2),
        ("miller product", lambda g1, g2, f: eng.miller_product(g1, g2), 0),
        ("product check", lambda g1, g2, f: eng.pairing_product_check(g1, g2), 1),
        ("pairing check", lambda g1, g2, f: eng.pairing_check(g1, g2, 2), 0),
        ("g1 is_valid", lambda g1, g2, f: eng.g1_is_valid(g1), 0),
        ("g2 is_valid", lambda g1, g2, f: eng.g2_is_valid(g2), 1),
        ("g1 mul", lambda g1, g2, f: eng.g1_mul(g1[:16], sc if isinstance(g1, np.ndarray) else _t(sc)), 0),
        ("g2 mul", lambda g1, g2, f: eng.g2_mul(g2[:16], sc if isinstance(g2, np.ndarray) else _t(sc)), 1),
        ("g1 add", lambda g1, g2, f: eng.g1_add(g1[:8], g1[:8]), 0),
        ("g2 add", lambda g1, g2, f: eng.g2_add(g2[8:16], g2[:8]), 1),
        ("g1 msm", lambda g1, g2, f: eng.g1_msm(g1[:16], sc if isinstance(g1, np.ndarray) else _t(sc)), 0),
        ("g2 msm", lambda g1, g2, f: eng.g2_msm(g2[:16], sc if isinstance(g2, np.ndarray) else _t(sc)), 1),
    ]
    eng.set_validate(True)
    try:
        assert eng.take_validation_status() is False
        for name, call, which in calls:
            bad = (b1 if which == 0 else G1, b2 if which == 1 else G2, bml if which == 2 else ml)
            call(G1, G2, ml)                                                      # canonical, host: the word stays 0
            assert eng.take_validation_status() is False, name
            with pytest.raises(_lib.ZkpError) as ei:
                call(*bad)
            assert ei.value.status == ERR_NONCANONICAL and b"input limbs >= p" in eng._lib.zkp_last_error(eng._h), name
            assert eng.take_validation_status() is False, name                   # the host flavour does not write the word
            call(_t(G1), _t(G2), _t(ml))                                          # canonical, device
            assert eng.take_validation_status() is False, name
            call(*(_t(a) for a in bad))                                           # non-canonical, device: no error, the word is set
            assert eng.take_validation_status() is True, name
    finally:
        eng.set_validate(False)
