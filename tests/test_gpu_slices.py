"""The slice loops of the G1 NTT, FK20 (csrc/zkp_fk20.hip) and the KZG opening (csrc/zkp_poly.hip) on one MI355X (run with -m gpu): every
call here is the smallest that crosses a slice boundary of its entry point and ends in a short last slice, its inputs and expected bytes
are assembled from a small pool by a pseudo-random index sequence (tests/slice_pools.py), and tests/test_slices_cpu.py has shown without
a GPU that a slice which took offset 0, the previous slice's offset, or another slice's rows in ANY operand cannot give these bytes.
Every comparison is byte for byte; a failure names the first wrong item, its slice and its place in the slice."""
import numpy as np
import pytest

import fk20_replay_cases as frc
import poly_model as pm
import replay_cases as rc
import slice_pools as sp
from replay_cases import fr_rows

pytestmark = pytest.mark.gpu
R = pm.R


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    """makes the verifier's setup; never the engine under test"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def to_host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.ascontiguousarray(t)


def same(call, got, what):
    """got: name -> array or tensor, for every expected output of the call"""
    assert set(got) == set(call.outputs), what
    for name, (want, per) in call.outputs.items():
        g = to_host(got[name])
        assert g.nbytes == want.nbytes, (what, name, g.shape, want.shape)
        g = g.view(want.dtype).reshape(want.shape)
        if g.tobytes() != want.tobytes():
            pytest.fail("%s: output %s differs, first at %r" % (what, name, sp.first_difference(g, want, per, call)))


# ------------------------------------------------------------------------------------------------------------------- the G1 NTT
@pytest.mark.parametrize("flags", [0, pm.INVERSE | pm.BITREV])
def test_g1_ntt_three_slices_of_different_vectors(eng, flags):
    """N = 8, 2 * 32768 + 5 vectors: flags 0 loads bit-reversed and stores natural, INVERSE | BITREV loads and stores natural and scales.
    The host flavour out of place, the device flavour in place over points and flags"""
    call = sp.ntt_call(flags)
    inverse, bitrev = bool(flags & pm.INVERSE), bool(flags & pm.BITREV)
    pts, inf = call.arg("points"), call.arg("inf")
    assert inf.any()
    out, out_inf = eng.g1_ntt(pts, sp.NTT_LOG2, inverse=inverse, bitrev=bitrev, inf=inf)
    same(call, dict(out=out, out_inf=out_inf), "g1_ntt flags %d (host)" % flags)
    tp, ti = to_dev(pts), to_dev(inf)
    to, toi = eng.g1_ntt(tp, sp.NTT_LOG2, inverse=inverse, bitrev=bitrev, inf=ti, out=tp, out_inf=ti)
    assert to is tp and toi is ti
    same(call, dict(out=to, out_inf=toi), "g1_ntt flags %d (dev, in place)" % flags)


def test_g1_ntt_three_slices_without_input_flags(eng):
    """inf = NULL across two boundaries, on vectors that differ from slice to slice (no identity entry in any input)"""
    call = sp.ntt_call(0, finite=True)
    assert not call.arg("inf").any()
    to, toi = eng.g1_ntt(to_dev(call.arg("points")), sp.NTT_LOG2)
    same(call, dict(out=to, out_inf=toi), "g1_ntt inf = None (dev)")


# ------------------------------------------------------------------------------------------------------------------- FK20
@pytest.mark.parametrize("bitrev", [False, True])
def test_fk20_two_slices_of_different_polynomials(eng, bitrev):
    """N = 4, 32768 + 3 polynomials: the coefficient, proof and flag offsets of the second slice, whose three polynomials (a constant one
    among them) occur nowhere in the first"""
    call = sp.fk20_call(bitrev)
    setup, sinf = frc.fk20_setup_for(sp.FK20_LOG2)
    coeffs = call.arg("coeffs")
    proof, inf = eng.kzg_fk20(setup, sinf, coeffs, sp.FK20_LOG2, bitrev)
    same(call, dict(proof=proof, inf=inf), "kzg_fk20 bitrev %d (host)" % bitrev)
    tp, ti = eng.kzg_fk20(to_dev(setup), to_dev(sinf), to_dev(coeffs), sp.FK20_LOG2, bitrev)
    same(call, dict(proof=tp, inf=ti), "kzg_fk20 bitrev %d (dev)" % bitrev)


# ------------------------------------------------------------------------------------------------------------------- the opening
@pytest.mark.parametrize("bitrev", [False, True])
def test_kzg_open_two_slices_with_a_short_last_one(eng, helper, bitrev):
    """N = 2^10, 4096 + 3 openings: the last slice has its own EvalLayout (another `den` offset, one sum block).  The device flavour on
    both orders, the host flavour on the bit-reversed one; the verifier on the three proofs of the tail"""
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import synthetic
    call = sp.open_call(bitrev)
    p = call.pool
    lag, evals, zs = p["setup"].lagrange_g1, call.arg("evals"), call.arg("z")
    ty, tp, ti = eng.kzg_open(to_dev(lag), to_dev(evals), to_dev(zs), sp.OPEN_LOG2, bitrev)
    same(call, dict(y=ty, proof=tp, inf=ti), "kzg_open bitrev %d (dev)" % bitrev)
    y, proof, inf = to_host(ty), to_host(tp).view(np.uint64), to_host(ti)
    if bitrev:
        y, proof, inf = eng.kzg_open(lag, evals, zs, sp.OPEN_LOG2, bitrev)
        same(call, dict(y=y, proof=proof, inf=inf), "kzg_open bitrev %d (host)" % bitrev)
    # what the last slice produced, against commitments made from the same trapdoor
    t = slice(call.n - call.tail, call.n)
    ids = list(sp.OPEN_TAIL)
    vs = z.KzgSetup(synthetic.G1_GENERATOR, synthetic.G2_GENERATOR, rc._g2(helper, [sp.TAU])[0])
    c, cinf = p["commit"][ids], p["cinf"][ids]
    y_t = np.ascontiguousarray(y.view(np.uint64).reshape(-1, 4)[t])
    args = dict(engine=helper, inf_c=cinf, inf_proof=np.ascontiguousarray(inf[t]))
    assert z.kzg_verify_batch(vs, c, zs[t], y_t, np.ascontiguousarray(proof.reshape(-1, 12)[t]), **args) is True
    y_bad = fr_rows([(int.from_bytes(y_t[k].tobytes(), "little") + (k == 2)) % R for k in range(3)])
    assert z.kzg_verify_batch(vs, c, zs[t], y_bad, np.ascontiguousarray(proof.reshape(-1, 12)[t]), **args) is False
