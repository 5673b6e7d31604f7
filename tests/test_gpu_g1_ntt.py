"""The batched G1 NTT on one MI355X (zkp_g1_ntt_batch, include/zkp_fk20.h): output points and flags byte for byte against the transform
of the exponents on Python integers and one oracle multiplication of the generator per output (tests/fk20_replay_cases.py), for every
flag combination, in place and out of place, through the host and the device flavour; forward then inverse gives the input back.  The
sizes: 0 the identity map, 1 only the stage that multiplies nothing, 2 and 3 the first twiddled stages, 6 half a wavefront of
butterflies, 7 exactly one, 8 two workgroups; three vectors of 64 leave a partial last wavefront.  Run with -m gpu."""
import ctypes
import random

import numpy as np
import pytest

import fk20_replay_cases as frc
import poly_model as pm
import replay_cases as rc

pytestmark = pytest.mark.gpu
R = pm.R
SIZES = [0, 1, 2, 3, 6, 7, 8]


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def check_call(eng, kinds, log2_n, flags, rng, what):
    inverse, bitrev = bool(flags & pm.INVERSE), bool(flags & pm.BITREV)
    pts, inf, want, want_inf = frc.ntt_io([frc.make_vector(k, log2_n, flags, rng) for k in kinds], log2_n, flags)
    # host flavour out of place, device flavour in place - and the other way round for the odd flags
    host_in_place = bool(flags & 1)
    if host_in_place:
        out, out_inf = pts.copy(), inf.copy()
        eng.g1_ntt(out, log2_n, inverse=inverse, bitrev=bitrev, inf=out_inf, out=out, out_inf=out_inf)
    else:
        out, out_inf = eng.g1_ntt(pts, log2_n, inverse=inverse, bitrev=bitrev, inf=inf)
    assert out_inf.tobytes() == want_inf.tobytes() and out.tobytes() == want.tobytes(), (what, "host")
    tp, ti = to_dev(pts), to_dev(inf)
    if host_in_place:
        to, toi = eng.g1_ntt(tp, log2_n, inverse=inverse, bitrev=bitrev, inf=ti)
    else:
        to, toi = eng.g1_ntt(tp, log2_n, inverse=inverse, bitrev=bitrev, inf=ti, out=tp, out_inf=ti)
        assert to is tp and toi is ti
    assert toi.cpu().numpy().tobytes() == want_inf.tobytes() and to.cpu().numpy().tobytes() == want.tobytes(), (what, "dev")
    # the inverse map under the same other flag gives the input bytes back
    back, back_inf = eng.g1_ntt(out, log2_n, inverse=not inverse, bitrev=bitrev, inf=out_inf)
    assert back_inf.tobytes() == inf.tobytes() and back.tobytes() == pts.tobytes(), (what, "round trip")


@pytest.mark.parametrize("flags", [0, pm.INVERSE, pm.BITREV, pm.INVERSE | pm.BITREV])
@pytest.mark.parametrize("n_vec", [1, 3])
@pytest.mark.parametrize("log2_n", SIZES)
def test_transform_equals_the_transform_of_the_exponents(eng, log2_n, n_vec, flags):
    rng = random.Random(0x61A7 + 100 * log2_n + 10 * n_vec + flags)
    kinds = [frc.VECTOR_KINDS[(flags + log2_n + 2 * j) % 5] for j in range(n_vec)]
    check_call(eng, kinds, log2_n, flags, rng, (log2_n, n_vec, flags, kinds))


@pytest.mark.parametrize("flags", [0, pm.INVERSE | pm.BITREV])
@pytest.mark.parametrize("log2_n", [2, 6, 7])
def test_every_kind_of_vector_in_one_call(eng, log2_n, flags):
    """random exponents, identity entries through the flags, an all-identity vector, a constant vector (every stage meets A = T and
    A = -T; every output but slot 0 is the identity) and a vector whose transform is a single non-zero entry, side by side"""
    rng = random.Random(0x5A1 + log2_n + flags)
    check_call(eng, list(frc.VECTOR_KINDS), log2_n, flags, rng, (log2_n, flags))
    n = 1 << log2_n
    const = frc.make_vector("constant", log2_n, flags, rng)
    out = pm.ntt_flags(const, log2_n, flags)
    assert out[0] != 0 and not any(out[1:])
    spike = pm.ntt_flags(frc.make_vector("spike", log2_n, flags, rng), log2_n, flags)
    assert sum(1 for v in spike if v) == 1 and len(spike) == n


def test_flags_may_be_null_and_a_sliced_call_equals_its_slices(eng):
    """inf = NULL means every point is finite; 2^18 + 2 points of size-2 vectors run in two slices"""
    rng = random.Random(0x511CE)
    v = [frc.make_vector("random", 3, 0, rng) for _ in range(2)]
    pts, inf, want, want_inf = frc.ntt_io(v, 3, 0)
    assert not inf.any()
    out, out_inf = eng.g1_ntt(pts, 3)
    assert out.tobytes() == want.tobytes() and out_inf.tobytes() == want_inf.tobytes()
    # many copies of one size-2 vector: every slice gives the same two points
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    p2, _ = rc.expect_points(1, [a, b])
    w2, wi2 = rc.expect_points(1, [(a + b) % R, (a - b) % R])
    n_vec = (1 << 17) + 1
    out, out_inf = eng.g1_ntt(np.tile(p2, (n_vec, 1)), 1)
    assert not out_inf.any() and out.tobytes() == np.tile(w2, (n_vec, 1)).tobytes()


def test_argument_errors_and_validation_mode():
    from zkvm_pairings_amd import PairingEngine, ZkpError
    rng = random.Random(0xA26)
    e = PairingEngine(0, validate=True)
    try:
        pts, inf, want, want_inf = frc.ntt_io([frc.make_vector("holes", 2, 0, rng)], 2, 0)
        out, out_inf = e.g1_ntt(pts, 2, inf=inf)
        assert out.tobytes() == want.tobytes() and out_inf.tobytes() == want_inf.tobytes()
        e.g1_ntt(to_dev(pts), 2, inf=to_dev(inf))
        assert e.take_validation_status() is False
        bad = pts.copy()
        bad[1, :6] = np.array([(rc.P >> (64 * i)) & rc.M64 for i in range(6)], dtype=np.uint64)      # x = p
        with pytest.raises(ZkpError) as ei:
            e.g1_ntt(bad, 2, inf=inf)
        assert ei.value.status == -4
        e.g1_ntt(to_dev(bad), 2, inf=to_dev(inf))
        assert e.take_validation_status() is True and e.take_validation_status() is False
        lib, h = e._lib, e._h
        buf = np.zeros((64, 12), dtype=np.uint64)
        p = ctypes.c_void_p(buf.ctypes.data)
        assert lib.zkp_g1_ntt_batch(h, p, p, 1, 21, 0, p, p) == -1 and lib.zkp_g1_ntt_batch(h, p, p, 5, 20, 0, p, p) == -1
        assert lib.zkp_g1_ntt_batch(h, p, p, (1 << 22) + 1, 0, 0, p, p) == -1
        for flags in (4, 5, 8, -1):
            assert lib.zkp_g1_ntt_batch(h, p, p, 1, 2, flags, p, p) == -1 and lib.zkp_g1_ntt_batch_dev(h, p, p, 1, 2, flags, p, p, None) == -1, flags
        for hole in (0, 2, 3):                       # points, out, out_inf; inf alone may be null
            args = [p] * 4
            args[hole] = None
            assert lib.zkp_g1_ntt_batch(h, args[0], args[1], 1, 2, 0, args[2], args[3]) == -1, hole
            assert lib.zkp_g1_ntt_batch_dev(h, args[0], args[1], 1, 2, 0, args[2], args[3], None) == -1, hole
        assert lib.zkp_g1_ntt_batch(None, p, p, 1, 2, 0, p, p) == -1
        assert lib.zkp_g1_ntt_batch(h, None, None, 0, 20, 3, None, None) == 0 and lib.zkp_g1_ntt_batch_dev(h, None, None, 0, 3, 0, None, None, None) == 0
        with pytest.raises(ValueError):
            e.g1_ntt(pts[:3], 2)
    finally:
        e.close()
