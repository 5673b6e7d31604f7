"""FK20 on one MI355X (zkp_kzg_fk20_setup, zkp_kzg_fk20_batch, include/zkp_fk20.h; kzg_lagrange_setup through the inverse G1 NTT): the
setup and the N proofs of a polynomial byte for byte against the values derived from a known tau - Python integers and one oracle
multiplication of the generator each (tests/fk20_replay_cases.py) -, against the single-point opening of the same polynomial at every
domain point, and the verifier's verdict on what was produced; the host and the device flavour.  Run with -m gpu."""
import ctypes
import random

import numpy as np
import pytest

import fk20_model as fm
import fk20_replay_cases as frc
import poly_model as pm
import poly_replay_cases as prc
import replay_cases as rc
from replay_cases import fr_rows

pytestmark = pytest.mark.gpu
R = pm.R
TAU = frc.TAU


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    """the engine the Lagrange setups and the verifier's setup are made with"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def verifier_setup(helper):
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import synthetic
    return z.KzgSetup(synthetic.G1_GENERATOR, synthetic.G2_GENERATOR, rc._g2(helper, [TAU])[0])


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


@pytest.mark.parametrize("log2_n", [0, 1, 2, 3, 6, 8])
def test_setup_equals_the_transform_of_the_setup_vector(eng, log2_n):
    import zkvm_pairings_amd as z
    want, want_inf = frc.fk20_setup_for(log2_n)
    mono = frc.monomial_for(log2_n)
    st = z.kzg_fk20_setup(mono, engine=eng)
    assert st.log2_n == log2_n and st.inf.tobytes() == want_inf.tobytes() and st.points.tobytes() == want.tobytes()
    tp, ti = eng.kzg_fk20_setup(to_dev(mono), log2_n)
    assert ti.cpu().numpy().tobytes() == want_inf.tobytes() and tp.cpu().numpy().tobytes() == want.tobytes()
    if log2_n == 0:
        assert want_inf.all()


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("log2_n", [0, 1, 2, 3, 6, 8])
def test_proofs_against_tau_the_single_point_opening_and_the_verifier(eng, helper, verifier_setup, log2_n, n, bitrev):
    import zkvm_pairings_amd as z
    rng = random.Random(0xF420 + 100 * log2_n + 10 * n + bitrev)
    big_n = 1 << log2_n
    kinds = [frc.POLY_KINDS[(log2_n + bitrev + 2 * j) % 5] for j in range(n)]
    if n == 3:
        kinds[0] = "random"
    polys = [frc.make_poly(k, big_n, rng) for k in kinds]
    what = (log2_n, n, bitrev, kinds)
    setup, sinf = frc.fk20_setup_for(log2_n)
    want, want_inf = frc.proofs_for(polys, log2_n, bitrev)
    coeffs = fr_rows([v for f in polys for v in f])
    proof, inf = z.kzg_open_domain_batch(z.Fk20Setup(setup, sinf, log2_n), coeffs, bitrev=bitrev, engine=eng)
    assert proof.shape == (n, big_n, 12) and inf.shape == (n, big_n)
    assert inf.tobytes() == want_inf.tobytes() and proof.tobytes() == want.tobytes(), what
    tp, ti = eng.kzg_fk20(to_dev(setup), to_dev(sinf), to_dev(coeffs), log2_n, bitrev)
    assert ti.cpu().numpy().tobytes() == want_inf.tobytes() and tp.cpu().numpy().tobytes() == want.tobytes(), what
    for j, k in enumerate(kinds):
        if k in ("zero", "constant"):
            assert want_inf[j * big_n:(j + 1) * big_n].all(), what
    st = prc.setup_for(helper, log2_n, bitrev)
    evals = [pm.ntt(f, log2_n, bitrev=bitrev) for f in polys]
    if big_n <= 64:
        # the path the library had before: the same polynomial opened at each domain point, one opening per (polynomial, slot)
        ev = fr_rows([v for e in evals for _ in range(big_n) for v in e])
        zs = fr_rows([st.slot_domain[m] for _ in range(n) for m in range(big_n)])
        y1, p1, i1 = z.kzg_open_batch(st.lagrange_g1, ev, zs, bitrev=bitrev, engine=eng)
        assert y1.tobytes() == fr_rows([v for e in evals for v in e]).tobytes(), what
        assert i1.tobytes() == inf.tobytes() and p1.tobytes() == proof.tobytes(), what
    # the verifier accepts all N proofs of polynomial 0 against its commitment, and rejects them once one y is off by one
    c, cinf = rc.expect_points(1, [fm.horner(polys[0], TAU)] * big_n)
    zs, ys = fr_rows(st.slot_domain), fr_rows(evals[0])
    assert z.kzg_verify_batch(verifier_setup, c, zs, ys, proof[0], engine=eng, inf_c=cinf, inf_proof=inf[0]) is True, what
    bad = list(evals[0])
    bad[big_n // 2] = (bad[big_n // 2] + 1) % R
    assert z.kzg_verify_batch(verifier_setup, c, zs, fr_rows(bad), proof[0], engine=eng, inf_c=cinf, inf_proof=inf[0]) is False, what


def test_every_kind_of_polynomial_in_one_call(eng):
    rng = random.Random(0xA11)
    log2_n, big_n = 3, 8
    polys = [frc.make_poly(k, big_n, rng) for k in frc.POLY_KINDS]
    assert polys[4][1:big_n - 1] == [0] * (big_n - 2) and polys[4][0] and polys[4][-1]
    setup, sinf = frc.fk20_setup_for(log2_n)
    for bitrev in (False, True):
        want, want_inf = frc.proofs_for(polys, log2_n, bitrev)
        proof, inf = eng.kzg_fk20(setup, sinf, fr_rows([v for f in polys for v in f]), log2_n, bitrev)
        assert inf.tobytes() == want_inf.tobytes() and proof.tobytes() == want.tobytes(), bitrev
        assert want_inf.reshape(5, big_n)[1].all() and want_inf.reshape(5, big_n)[2].all() and not want_inf.reshape(5, big_n)[0].any()


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("log2_n", [0, 1, 2, 3, 6, 8])
def test_lagrange_setup_from_the_monomial_setup(eng, helper, log2_n, bitrev):
    import zkvm_pairings_amd as z
    st = prc.setup_for(helper, log2_n, bitrev)
    got = z.kzg_lagrange_setup(frc.monomial_for(log2_n), bitrev=bitrev, engine=eng)
    assert got.tobytes() == st.lagrange_g1.tobytes()
    assert got.tobytes() == rc.expect_points(1, st.lagrange_tau)[0].tobytes()


def test_validation_mode_and_argument_errors():
    from zkvm_pairings_amd import PairingEngine, ZkpError
    rng = random.Random(0x0AF)
    setup, sinf = frc.fk20_setup_for(2)
    mono = frc.monomial_for(2)
    e = PairingEngine(0, validate=True)
    try:
        polys = [frc.make_poly("random", 4, rng) for _ in range(2)]
        coeffs = fr_rows([v for f in polys for v in f])
        want, want_inf = frc.proofs_for(polys, 2, False)
        proof, inf = e.kzg_fk20(setup, sinf, coeffs, 2)
        assert proof.tobytes() == want.tobytes() and inf.tobytes() == want_inf.tobytes()
        e.kzg_fk20(to_dev(setup), to_dev(sinf), to_dev(coeffs), 2)
        e.kzg_fk20_setup(to_dev(mono), 2)
        assert e.take_validation_status() is False
        bad = coeffs.copy()
        bad[7] = fr_rows([R])[0]
        with pytest.raises(ZkpError) as ei:
            e.kzg_fk20(setup, sinf, bad, 2)
        assert ei.value.status == -4
        e.kzg_fk20(to_dev(setup), to_dev(sinf), to_dev(bad), 2)
        assert e.take_validation_status() is True and e.take_validation_status() is False
        lib, h = e._lib, e._h
        buf = np.zeros((64, 12), dtype=np.uint64)
        p = ctypes.c_void_p(buf.ctypes.data)
        assert lib.zkp_kzg_fk20_batch(h, p, p, p, 1, 20, 0, p, p) == -1 and lib.zkp_kzg_fk20_batch(h, p, p, p, 5, 19, 0, p, p) == -1
        assert lib.zkp_kzg_fk20_batch(h, p, p, p, (1 << 21) + 1, 0, 0, p, p) == -1
        for flags in (1, 3, 4, 8, -1):
            assert lib.zkp_kzg_fk20_batch(h, p, p, p, 1, 2, flags, p, p) == -1 and lib.zkp_kzg_fk20_batch_dev(h, p, p, p, 1, 2, flags, p, p, None) == -1, flags
        for hole in (0, 2, 3, 4):                    # setup, coeffs, out_proof, out_inf; the setup's flags alone may be null
            args = [p] * 5
            args[hole] = None
            assert lib.zkp_kzg_fk20_batch(h, args[0], args[1], args[2], 1, 2, 0, args[3], args[4]) == -1, hole
            assert lib.zkp_kzg_fk20_batch_dev(h, args[0], args[1], args[2], 1, 2, 0, args[3], args[4], None) == -1, hole
        assert lib.zkp_kzg_fk20_batch(None, p, p, p, 1, 2, 0, p, p) == -1
        assert lib.zkp_kzg_fk20_batch(h, None, None, None, 0, 19, 2, None, None) == 0
        assert lib.zkp_kzg_fk20_batch_dev(h, None, None, None, 0, 3, 0, None, None, None) == 0
        assert lib.zkp_kzg_fk20_setup(h, p, 20, p, p) == -1 and lib.zkp_kzg_fk20_setup_dev(h, p, 20, p, p, None) == -1
        for hole in range(3):
            args = [p] * 3
            args[hole] = None
            assert lib.zkp_kzg_fk20_setup(h, args[0], 2, args[1], args[2]) == -1 and lib.zkp_kzg_fk20_setup_dev(h, args[0], 2, args[1], args[2], None) == -1, hole
        assert lib.zkp_kzg_fk20_setup(None, p, 2, p, p) == -1
        with pytest.raises(ValueError):
            e.kzg_fk20(setup[:7], sinf[:7], coeffs, 2)
    finally:
        e.close()


def test_plain_c_consumer_runs(tmp_path):
    """integration/c/zkp_fk20.c: the header and three of the calls from plain C (no Python, no torch types)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "zkvm_pairings_amd")
    exe = str(tmp_path / "zkp_fk20")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "integration", "c", "zkp_fk20.c"), "-L", libdir,
                           "-lzkp_pairings", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "zkp_fk20 ok" in out.stdout, out.stdout + out.stderr
