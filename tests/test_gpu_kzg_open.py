"""The producer side of KZG on one MI355X (zkp_kzg_open_batch, include/zkp_poly.h; kzg_commit_batch through the shared-bases MSM): y, the
proof and the commitment against the values derived from a known tau - Python integers and one oracle multiplication of the generator
each (tests/poly_replay_cases.py) -, the verifier's verdict on what was produced, the host and the device flavour.  Run with -m gpu."""
import ctypes
import random

import numpy as np
import pytest

import poly_replay_cases as prc
import replay_cases as rc
from replay_cases import fr_rows

pytestmark = pytest.mark.gpu
R = prc.R


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    """the engine the setups are made with: the engine under test sees only the calls under test"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def verifier_setup(helper):
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import synthetic
    return z.KzgSetup(synthetic.G1_GENERATOR, synthetic.G2_GENERATOR, rc._g2(helper, [prc.TAU])[0])


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def z_kinds(big_n):
    return [k for k in prc.Z_KINDS if not (k == "slot1" and big_n < 2) and not (k == "slotlast" and big_n < 3)]


def batches(n, big_n):
    """(polynomial kinds, point kinds) of the calls of one test: every kind of polynomial meets every kind of point that exists for the
    size, n pairs per call (the last call is filled up from the start); one more call of random polynomials has the in-domain slots
    side by side"""
    pairs = [(pk, zk) for pk in prc.POLY_KINDS for zk in z_kinds(big_n)]
    out = []
    for start in range(0, len(pairs), n):
        chunk = (pairs + pairs)[start:start + n]
        out.append(([p for p, _ in chunk], [k for _, k in chunk]))
    if n > 1 and big_n > 1:
        out.append((["random"] * n, (["slot0", "slot1", "outside", "slotlast" if big_n > 2 else "zero", "zero"])[:n]))
    return out


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("log2_n", [0, 1, 2, 6, 8, 9, 12])
def test_open_and_commit_against_the_values_derived_from_tau(eng, helper, verifier_setup, log2_n, n, bitrev):
    import zkvm_pairings_amd as z
    rng = random.Random(0x09E4 + 100 * log2_n + 10 * n + bitrev)
    st = prc.setup_for(helper, log2_n, bitrev)
    for which, (pk, zk) in enumerate(batches(n, st.n)):
        polys = [prc.make_poly(k, st.n, rng) for k in pk]
        zs = [prc.make_z(k, st, rng) for k in zk]
        d = prc.opening(st, polys, zs)
        what = (log2_n, n, bitrev, pk, zk)
        y, proof, inf = z.kzg_open_batch(st.lagrange_g1, d["evals"], d["z"], bitrev=bitrev, engine=eng)
        assert y.tobytes() == d["y"].tobytes(), what
        assert inf.tobytes() == d["inf"].tobytes() and proof.tobytes() == d["proof"].tobytes(), what
        ty, tp, ti = eng.kzg_open(to_dev(st.lagrange_g1), to_dev(d["evals"]), to_dev(d["z"]), log2_n, bitrev)
        assert ty.cpu().numpy().tobytes() == d["y"].tobytes() and tp.cpu().numpy().tobytes() == d["proof"].tobytes(), what
        assert ti.cpu().numpy().tobytes() == d["inf"].tobytes(), what
        c, cinf = z.kzg_commit_batch(st.lagrange_g1, d["evals"], engine=eng)
        assert c.tobytes() == d["commit"].tobytes() and np.asarray(cinf).tobytes() == d["cinf"].tobytes(), what
        if which == 0:
            # the verifier accepts what was produced, and rejects it once one value is off by one
            assert z.kzg_verify_batch(verifier_setup, c, d["z"], y, proof, engine=eng, inf_c=cinf, inf_proof=inf) is True, what
            y_bad = fr_rows([(int.from_bytes(y[0].tobytes(), "little") + 1) % R]
                            + [int.from_bytes(y[j].tobytes(), "little") for j in range(1, n)])
            assert z.kzg_verify_batch(verifier_setup, c, d["z"], y_bad, proof, engine=eng, inf_c=cinf, inf_proof=inf) is False, what


def test_every_kind_of_polynomial_meets_every_kind_of_point():
    for big_n in (1, 2, 4, 64):
        for n in (1, 3, 5):
            calls = batches(n, big_n)
            assert all(len(pk) == len(zk) == n for pk, zk in calls)
            seen = {pair for pk, zk in calls for pair in zip(pk, zk)}
            assert seen >= {(p, k) for p in prc.POLY_KINDS for k in z_kinds(big_n)}, (big_n, n)
            if n > 1 and big_n > 1:
                assert len({k for k in calls[-1][1] if k.startswith("slot")}) >= 2


def test_blob_pipeline_ntt_commit_open_verify(eng, helper, verifier_setup):
    """coefficients -> evaluations (NTT, bit-reversed as blobs are stored) -> commitments and openings -> the blob verifier"""
    import zkvm_pairings_amd as z
    rng = random.Random(0xB10B)
    log2_n, n = 12, 3
    st = prc.setup_for(helper, log2_n, True)
    polys = [[rng.randrange(R) for _ in range(st.n)] for _ in range(n)]
    zs = [rng.randrange(R), st.slot_domain[5], 0]
    evals = eng.fr_ntt(fr_rows([v for p in polys for v in p]), log2_n, bitrev=True)
    c, cinf = z.kzg_commit_batch(st.lagrange_g1, evals, engine=eng)
    y, proof, inf = z.kzg_open_batch(st.lagrange_g1, evals, fr_rows(zs), bitrev=True, engine=eng)
    assert y.tobytes() == fr_rows([prc.horner(p, x) for p, x in zip(polys, zs)]).tobytes() and not cinf.any() and not inf.any()
    assert z.kzg_verify_blob_batch(verifier_setup, evals.reshape(n, st.n, 4), c, fr_rows(zs), proof, bitrev=True, engine=eng) is True
    proof[[0, 1]] = proof[[1, 0]]
    assert z.kzg_verify_blob_batch(verifier_setup, evals.reshape(n, st.n, 4), c, fr_rows(zs), proof, bitrev=True, engine=eng) is False


def test_validation_mode_and_argument_errors(helper):
    from zkvm_pairings_amd import PairingEngine, ZkpError
    rng = random.Random(0x0AE)
    st = prc.setup_for(helper, 2, False)
    e = PairingEngine(0, validate=True)
    try:
        d = prc.opening(st, [prc.make_poly("random", 4, rng) for _ in range(2)], [prc.make_z("outside", st, rng), st.slot_domain[3]])
        y, proof, inf = e.kzg_open(st.lagrange_g1, d["evals"], d["z"], 2)
        assert y.tobytes() == d["y"].tobytes() and proof.tobytes() == d["proof"].tobytes()
        e.kzg_open(to_dev(st.lagrange_g1), to_dev(d["evals"]), to_dev(d["z"]), 2)
        assert e.take_validation_status() is False
        for name, row in (("evals", 7), ("z", 1)):
            bad = {k: v.copy() for k, v in d.items()}
            bad[name][row] = fr_rows([R])[0]
            with pytest.raises(ZkpError) as ei:
                e.kzg_open(st.lagrange_g1, bad["evals"], bad["z"], 2)
            assert ei.value.status == -4, name
            e.kzg_open(to_dev(st.lagrange_g1), to_dev(bad["evals"]), to_dev(bad["z"]), 2)
            assert e.take_validation_status() is True and e.take_validation_status() is False, name
        lib, h = e._lib, e._h
        buf = np.zeros((64, 12), dtype=np.uint64)
        p = ctypes.c_void_p(buf.ctypes.data)
        assert lib.zkp_kzg_open_batch(h, p, p, p, 1, 21, 0, p, p, p) == -1 and lib.zkp_kzg_open_batch(h, p, p, p, 1, 2, 2, p, p, p) == -1
        assert lib.zkp_kzg_open_batch(h, p, p, p, 17, 20, 0, p, p, p) == -1 and lib.zkp_kzg_open_batch(h, p, p, p, (1 << 24) + 1, 0, 0, p, p, p) == -1
        for hole in range(6):
            args = [p] * 6
            args[hole] = None
            assert lib.zkp_kzg_open_batch(h, args[0], args[1], args[2], 1, 2, 0, args[3], args[4], args[5]) == -1, hole
            assert lib.zkp_kzg_open_batch_dev(h, args[0], args[1], args[2], 1, 2, 0, args[3], args[4], args[5], None) == -1, hole
        assert lib.zkp_kzg_open_batch(None, p, p, p, 1, 2, 0, p, p, p) == -1
        assert lib.zkp_kzg_open_batch(h, None, None, None, 0, 20, 1, None, None, None) == 0
        assert lib.zkp_kzg_open_batch_dev(h, None, None, None, 0, 3, 0, None, None, None, None) == 0
        with pytest.raises(ValueError):
            e.kzg_open(st.lagrange_g1[:3], d["evals"], d["z"], 2)
    finally:
        e.close()
