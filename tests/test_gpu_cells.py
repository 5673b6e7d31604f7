"""The KZG cell proofs on one MI355X (zkp_kzg_cells_setup, zkp_kzg_cells_batch, zkp_kzg_cell_verify_batch, include/zkp_cells.h): the setup
and the M proofs of a polynomial byte for byte against the DEFINITION - the quotient by X^l - c^l on Python integers (tests/cells_model.py)
and one oracle multiplication of the generator per point (tests/cells_replay_cases.py) -, at every group size the planner takes, on the
edge inputs of the multiply-accumulate, across a slice boundary; the degenerate cell size against FK20; the round trip through the batch
verifier and the per-cell path; the host and the device flavour.  Run with -m gpu."""
import ctypes
import random

import numpy as np
import pytest

import cells_model as cm
import cells_replay_cases as crc
import cells_shapes
import fk20_replay_cases as frc
import poly_model as pm
import replay_cases as rc
import slice_pools as sp
from replay_cases import fr_rows

pytestmark = pytest.mark.gpu
R = pm.R
TAU = crc.TAU
# (log2_n, log2_l, log2_ext): (64, 4, 2), (64, 4, 1), (16, 16, 2) with k = 1, (8, 2, 2), (64, 1, 1)
SHAPES = [(6, 2, 1), (6, 2, 0), (4, 4, 1), (3, 1, 1), (6, 0, 0)]


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    """the engine [tau^l] g2 is made with"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def cell_setup(log2_n, log2_l):
    import zkvm_pairings_amd as z
    pts, inf = crc.cells_setup_for(log2_n, log2_l)
    return z.CellSetup(pts, inf, log2_n, log2_l)


@pytest.mark.parametrize("log2_n,log2_l", [(6, 2), (4, 4), (3, 1), (6, 0), (0, 0), (3, 0), (5, 4)])
def test_setup_equals_the_transforms_of_the_stride_vectors(eng, log2_n, log2_l):
    import zkvm_pairings_amd as z
    want, want_inf = crc.cells_setup_for(log2_n, log2_l)
    mono = crc.monomial_for(log2_n)
    st = z.kzg_cells_setup(mono, log2_l, engine=eng)
    assert (st.log2_n, st.log2_l) == (log2_n, log2_l) and st.inf.tobytes() == want_inf.tobytes() and st.points.tobytes() == want.tobytes()
    tp, ti = eng.kzg_cells_setup(to_dev(mono), log2_n, log2_l)
    assert ti.cpu().numpy().tobytes() == want_inf.tobytes() and tp.cpu().numpy().tobytes() == want.tobytes()
    if log2_l == log2_n:
        assert want_inf.all()                                                          # k = 1: nothing but identities
    if log2_l == 0:                                                                    # byte for byte what FK20's setup gives
        fk = z.kzg_fk20_setup(mono, engine=eng)
        assert fk.points.tobytes() == st.points.tobytes() and fk.inf.tobytes() == st.inf.tobytes()
        assert frc.fk20_setup_for(log2_n)[0].tobytes() == want.tobytes()


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=["N64-l4-e2", "N64-l4-e1", "N16-l16-e2", "N8-l2-e2", "N64-l1-e1"])
def test_proofs_against_the_definition(eng, shape, n, bitrev):
    import zkvm_pairings_amd as z
    log2_n, log2_l, log2_ext = shape
    rng = random.Random(0xCE11 + 1000 * log2_n + 100 * log2_l + 10 * n + 2 * log2_ext + bitrev)
    big_n, big_m = 1 << log2_n, 1 << (log2_n - log2_l + log2_ext)
    kinds = [frc.POLY_KINDS[(log2_n + bitrev + 2 * j) % 5] for j in range(n)]
    if n == 3:
        kinds[0] = "random"
    polys = [frc.make_poly(k, big_n, rng) for k in kinds]
    what = (shape, n, bitrev, kinds)
    st = cell_setup(log2_n, log2_l)
    want, want_inf = crc.proofs_for(polys, log2_n, log2_l, log2_ext, bitrev)
    coeffs = fr_rows([v for f in polys for v in f])
    proof, inf = z.kzg_cell_proofs_batch(st, coeffs, log2_ext=log2_ext, bitrev=bitrev, engine=eng)
    assert proof.shape == (n, big_m, 12) and inf.shape == (n, big_m)
    assert inf.tobytes() == want_inf.tobytes() and proof.tobytes() == want.tobytes(), what
    tp, ti = eng.kzg_cells(to_dev(st.points), to_dev(st.inf), to_dev(coeffs), log2_n, log2_l, log2_ext, bitrev)
    assert ti.cpu().numpy().tobytes() == want_inf.tobytes() and tp.cpu().numpy().tobytes() == want.tobytes(), what
    if log2_l == log2_n:
        assert want_inf.all(), what                                                    # k = 1: every proof infinite
    if log2_l == 0:                                                                    # l = 1: the FK20 single proofs of the same inputs
        fs, fi = frc.fk20_setup_for(log2_n)
        p1, i1 = eng.kzg_fk20(fs, fi, coeffs, log2_n, bitrev)
        assert p1.tobytes() == proof.tobytes() and i1.tobytes() == inf.tobytes(), what


@pytest.mark.parametrize("shape", cells_shapes.G_SHAPES, ids=["n%d-N%d-l%d-e%d-g%d" % (s[0], 1 << s[1], 1 << s[2], 1 << s[3], s[4]) for s in cells_shapes.G_SHAPES])
def test_every_group_size_the_planner_takes(eng, shape):
    """many polynomials assembled from a pool of seven (tests/slice_pools.py: draw, take), so that the expected points cost seven
    polynomials' worth of oracle multiplications; the zero polynomial and a constant among them"""
    n, log2_n, log2_l, log2_ext, _ = shape
    big_n, big_m, n_pool = 1 << log2_n, 1 << (log2_n - log2_l + log2_ext), 7
    rng = random.Random(0x6006 + n)
    polys = [frc.make_poly(k, big_n, rng) for k in ("random", "zero", "random", "constant", "ends", "random", "random")]
    pp, pi = crc.proofs_for(polys, log2_n, log2_l, log2_ext, True)
    idx = sp.draw(0x6007 + n, n, (5, 6), n_pool)
    coeffs = sp.take(fr_rows([v for f in polys for v in f]), n_pool, idx)
    st = cell_setup(log2_n, log2_l)
    proof, inf = eng.kzg_cells(st.points, st.inf, coeffs, log2_n, log2_l, log2_ext, True)
    assert proof.shape == (n * big_m, 12)
    assert inf.tobytes() == sp.take(pi, n_pool, idx).tobytes() and proof.tobytes() == sp.take(pp, n_pool, idx).tobytes(), shape


@pytest.mark.parametrize("tau", crc.EXCEPTIONAL_TAUS, ids=["tau1", "tau-1"])
@pytest.mark.parametrize("shape", cells_shapes.EXCEPTIONAL_SHAPES, ids=["g%d" % s[4] for s in cells_shapes.EXCEPTIONAL_SHAPES])
def test_additions_that_meet_equal_and_opposite_operands(eng, shape, tau):
    """The doubling and the P + (-P) case of k_cell_sum's addition and of the mixed addition inside k_cell_mac.  They need strides whose
    bases AND scalars agree up to sign: the setup of tau = 1 (every X_i the same) or tau = -1 (X_i alternating in sign), polynomials with
    equal coefficients or with sign blocks.  tests/test_cells_cpu.py counts the cases these very inputs reach on the model, and shows that
    equal coefficients under an ordinary tau reach none.  Many polynomials (g > 1 needs more than 2^16 lanes) come from a pool of seven."""
    n, log2_n, log2_l, log2_ext, g = shape
    n_pool = len(crc.EXCEPTIONAL_KINDS)
    polys = crc.exceptional_polys(log2_n, log2_l, g.bit_length() - 1, 0xE8C + n)
    want_s, want_si = crc.cells_setup_for(log2_n, log2_l, tau)
    got_s, got_si = eng.kzg_cells_setup(crc.monomial_for(log2_n, tau), log2_n, log2_l)
    assert got_si.tobytes() == want_si.tobytes() and got_s.tobytes() == want_s.tobytes()
    pp, pi = crc.proofs_for(polys, log2_n, log2_l, log2_ext, True, tau)
    idx = np.arange(n) if n <= n_pool else sp.draw(0xE8D + n, n, (5, 6), n_pool)
    coeffs = sp.take(fr_rows([v for f in polys for v in f]), n_pool, idx)
    proof, inf = eng.kzg_cells(got_s, got_si, coeffs, log2_n, log2_l, log2_ext, True)
    assert inf.tobytes() == sp.take(pi, n_pool, idx).tobytes() and proof.tobytes() == sp.take(pp, n_pool, idx).tobytes(), (shape, tau == 1)
    assert not pi.all()                                                                # not every proof is the identity


@pytest.mark.parametrize("bitrev", [False, True])
def test_edge_inputs_of_the_multiply_accumulate(eng, bitrev):
    """the zero polynomial, a constant, only f_{N-1}, all coefficients equal, two polynomials that are negatives of each other - in one
    call, at a shape with partials (N = 64, l = 4 runs g = 1: four partials per slot) and at one without (l = 1).  These make infinite
    accumulators and infinite partials; equal and opposite partials need the setups of the test above (under an ordinary tau equal
    coefficients do NOT give equal partials: the bases of the strides differ by powers of tau)"""
    rng = random.Random(0xED6E + bitrev)
    for log2_n, log2_l, log2_ext in ((6, 2, 1), (4, 0, 1), (4, 4, 0)):
        big_n = 1 << log2_n
        v, f = rng.randrange(1, R), [rng.randrange(1, R) for _ in range(big_n)]
        polys = [[0] * big_n, [v] + [0] * (big_n - 1), [0] * (big_n - 1) + [v], [v] * big_n, f, [(R - c) % R for c in f]]
        st = cell_setup(log2_n, log2_l)
        want, want_inf = crc.proofs_for(polys, log2_n, log2_l, log2_ext, bitrev)
        proof, inf = eng.kzg_cells(st.points, st.inf, fr_rows([c for p in polys for c in p]), log2_n, log2_l, log2_ext, bitrev)
        assert inf.tobytes() == want_inf.tobytes() and proof.tobytes() == want.tobytes(), (log2_n, log2_l, bitrev)
        big_m = proof.shape[0] // len(polys)
        assert want_inf[:2 * big_m].all()                                              # the zero polynomial and the constant: every proof infinite
        if log2_l < log2_n:
            assert not want_inf[3 * big_m:].all()


# ------------------------------------------------------------------------------------------------------------------- a slice boundary
@pytest.mark.parametrize("bitrev", [False, True])
def test_one_call_across_a_slice_boundary_with_a_short_last_slice(eng, bitrev):
    call = crc.slice_call(bitrev)
    assert len(call.starts) == 2 and call.tail == 3                      # test_cells_cpu.py holds the slice length to the planner's
    for name in ("proof", "inf"):                          # a build that computed slice 1 from offset 0 would not pass
        assert sp.reading(call, name, "zero").tobytes() != call.want(name).tobytes()
    st = cell_setup(crc.SLICE_LOG2, crc.SLICE_LOG2_L)
    proof, inf = eng.kzg_cells(st.points, st.inf, call.arg("coeffs"), crc.SLICE_LOG2, crc.SLICE_LOG2_L, crc.SLICE_EXT, bitrev)
    assert sp.first_difference(inf, call.want("inf"), 4, call) is None
    assert sp.first_difference(proof, call.want("proof"), 4, call) is None
    assert inf.tobytes() == call.want("inf").tobytes() and proof.tobytes() == call.want("proof").tobytes()


# ------------------------------------------------------------------------------------------------------------------- the round trip
def verifier_setup(helper, log2_l):
    return crc.monomial_for(log2_l), crc.g2_generator(), crc.tau_l_g2_for(helper, log2_l)


def test_round_trip_through_the_batch_verifier_and_the_per_cell_path(eng, helper):
    import zkvm_pairings_amd as z
    log2_n, log2_l, log2_ext = 6, 2, 1
    log2_d, big_m, l = log2_n + log2_ext, 1 << (log2_n - log2_l + log2_ext), 1 << log2_l
    rng = random.Random(0x7219)
    polys = [frc.make_poly("random", 1 << log2_n, rng) for _ in range(2)]
    cells, proof, inf = z.kzg_cells_and_proofs_batch(cell_setup(log2_n, log2_l), fr_rows([v for f in polys for v in f]), log2_ext=log2_ext, bitrev=True, engine=eng)
    assert cells.shape == (2, big_m, l, 4) and proof.shape == (2, big_m, 12)
    # the cells are rows of the Fr transform of the zero-padded coefficients, and the values of the definition
    ext = eng.fr_ntt(fr_rows([v for f in polys for v in list(f) + [0] * ((1 << log2_d) - len(f))]), log2_d, bitrev=True)
    assert cells.tobytes() == ext.tobytes()
    assert cells[1].tobytes() == fr_rows([v for row in cm.cell_values(polys[1], log2_n, log2_l, log2_ext, True) for v in row]).tobytes()
    mono, g2, tg2 = verifier_setup(helper, log2_l)
    com, cinf = rc.expect_points(1, [cm.horner(f, TAU) for f in polys])
    picks = [(j, m) for j in range(2) for m in range(big_m)]

    def arrays(picks):
        return (np.stack([com[j] for j, _ in picks]), np.array([m for _, m in picks], dtype=np.uint32), np.stack([cells[j, m] for j, m in picks]),
                np.stack([proof[j, m] for j, m in picks]), np.array([inf[j, m] for j, m in picks], dtype=np.uint8))
    c, idx, vals, prf, pinf = arrays(picks)
    verify = lambda c, idx, vals, prf, **kw: z.kzg_cell_verify_batch(mono, g2, tg2, c, idx, vals, prf, log2_d, bitrev=True, engine=eng, inf_proof=pinf, **kw)
    assert verify(c, idx, vals, prf) is True
    assert verify(c, idx, vals, prf, points_checked=True, vk_checked=True) is True
    dev = eng.kzg_cell_verify(*[to_dev(a) for a in (mono, g2, tg2, c, idx.astype(np.int32), vals.reshape(-1, 4), prf)], log2_d, log2_l, bitrev=True,
                              inf_proof=to_dev(pinf))
    assert int(dev.item()) == 1
    # the natural order as well: other cosets behind the same indices
    cells_n, proof_n, inf_n = z.kzg_cells_and_proofs_batch(cell_setup(log2_n, log2_l), fr_rows(polys[0]), log2_ext=log2_ext, bitrev=False, engine=eng)
    assert cells_n[0].tobytes() == fr_rows([v for row in cm.cell_values(polys[0], log2_n, log2_l, log2_ext, False) for v in row]).tobytes()
    assert z.kzg_cell_verify_batch(mono, g2, tg2, np.repeat(com[:1], big_m, axis=0), np.arange(big_m), cells_n[0], proof_n[0], log2_d, bitrev=False, engine=eng,
                                   inf_proof=inf_n[0]) is True
    # every single corruption fails, and the per-cell path names the cell
    short = [(0, 3), (1, 0), (1, big_m - 1), (0, 17), (1, 9)]
    c, idx, vals, prf, pinf = arrays(short)
    each = lambda c, idx, vals, prf: z.kzg_cell_verify_each(mono, g2, tg2, c, idx, vals, prf, log2_d, bitrev=True, engine=eng, inf_proof=pinf)
    assert verify(c, idx, vals, prf) is True and each(c, idx, vals, prf).all()
    for bad in range(len(short)):
        v2 = vals.copy()
        v2[bad, l - 1] = fr_rows([(cm.horner(polys[short[bad][0]], 5) + bad) % R])[0]
        i2 = idx.copy()
        i2[bad] ^= 1
        p2 = prf.copy()
        p2[bad] = prf[(bad + 1) % len(short)]
        c2 = c.copy()
        c2[bad] = com[1 - short[bad][0]]
        for what, args in (("value", (c, idx, v2, prf)), ("index", (c, i2, vals, prf)), ("proof", (c, idx, vals, p2)), ("commitment", (c2, idx, vals, prf))):
            assert verify(*args) is False, (what, bad)
            if bad in (0, len(short) - 1):
                assert each(*args).tolist() == [j != bad for j in range(len(short))], (what, bad)
    # not a verdict but a refusal: a value >= r, an index >= M, a zero pair of random words
    v2 = vals.copy()
    v2[2, 0] = fr_rows([R])[0]
    assert verify(c, idx, v2, prf) is False and not each(c, idx, v2, prf)[2]
    same = int.from_bytes(vals[2, 0].tobytes(), "little") + R                          # the true value's residue, another input: only the canonical check sees it
    assert same < 2 ** 256
    v3 = vals.copy()
    v3[2, 0] = fr_rows([same])[0]
    assert verify(c, idx, v3, prf) is False and verify(c, idx, v3, prf, points_checked=True, vk_checked=True) is False and not each(c, idx, v3, prf)[2]
    i2 = idx.copy()
    i2[1] += big_m
    assert verify(c, i2, vals, prf) is False and not each(c, i2, vals, prf)[1]
    rand = eng.rlc_random(len(short))
    rand[3] = 0
    assert verify(c, idx, vals, prf, rand=rand) is False
    assert z.kzg_cell_verify_batch(mono, g2, tg2, c[:0], idx[:0], vals[:0], prf[:0], log2_d, engine=eng) is True


def test_a_cell_with_an_infinite_proof_verifies(eng, helper):
    """k = 1: l = N, every proof is the identity and the cell is the whole polynomial on a coset"""
    import zkvm_pairings_amd as z
    log2_n = log2_l = 3
    rng = random.Random(0x1F1F)
    f = frc.make_poly("random", 8, rng)
    cells, proof, inf = z.kzg_cells_and_proofs_batch(cell_setup(log2_n, log2_l), fr_rows(f), log2_ext=1, bitrev=True, engine=eng)
    assert inf.all() and cells.shape == (1, 2, 8, 4)
    mono, g2, tg2 = verifier_setup(helper, log2_l)
    com = rc.expect_points(1, [cm.horner(f, TAU)] * 2)[0]
    args = (mono, g2, tg2, com, [0, 1], cells[0], proof[0], log2_n + 1)
    assert z.kzg_cell_verify_batch(*args, bitrev=True, engine=eng, inf_proof=inf[0]) is True
    assert z.kzg_cell_verify_each(*args, bitrev=True, engine=eng, inf_proof=inf[0]).all()
    swapped = np.ascontiguousarray(cells[0][::-1])
    assert z.kzg_cell_verify_batch(mono, g2, tg2, com, [0, 1], swapped, proof[0], log2_n + 1, bitrev=True, engine=eng, inf_proof=inf[0]) is False


def test_validation_mode_and_argument_errors():
    from zkvm_pairings_amd import PairingEngine, ZkpError
    rng = random.Random(0x0AF1)
    log2_n, log2_l = 3, 1
    setup, sinf = crc.cells_setup_for(log2_n, log2_l)
    mono = crc.monomial_for(log2_n)
    e = PairingEngine(0, validate=True)
    try:
        polys = [frc.make_poly("random", 8, rng) for _ in range(2)]
        coeffs = fr_rows([v for f in polys for v in f])
        want, want_inf = crc.proofs_for(polys, log2_n, log2_l, 1, False)
        proof, inf = e.kzg_cells(setup, sinf, coeffs, log2_n, log2_l, 1)
        assert proof.tobytes() == want.tobytes() and inf.tobytes() == want_inf.tobytes()
        e.kzg_cells(to_dev(setup), to_dev(sinf), to_dev(coeffs), log2_n, log2_l, 1)
        e.kzg_cells_setup(to_dev(mono), log2_n, log2_l)
        assert e.take_validation_status() is False
        bad = coeffs.copy()
        bad[9] = fr_rows([R])[0]
        with pytest.raises(ZkpError) as ei:
            e.kzg_cells(setup, sinf, bad, log2_n, log2_l, 1)
        assert ei.value.status == -4
        e.kzg_cells(to_dev(setup), to_dev(sinf), to_dev(bad), log2_n, log2_l, 1)
        assert e.take_validation_status() is True and e.take_validation_status() is False
        lib, h = e._lib, e._h
        buf = np.zeros((64, 12), dtype=np.uint64)
        p = ctypes.c_void_p(buf.ctypes.data)
        batch = lambda *a: (lib.zkp_kzg_cells_batch(h, *a), lib.zkp_kzg_cells_batch_dev(h, *a, None))
        assert batch(p, p, p, 1, 20, 0, 0, 0, p, p) == (-1, -1) and batch(p, p, p, 5, 19, 0, 0, 0, p, p) == (-1, -1)
        assert batch(p, p, p, 1, 2, 3, 0, 0, p, p) == (-1, -1) and batch(p, p, p, 1, 2, 1, 2, 0, p, p) == (-1, -1)
        assert batch(p, p, p, (1 << 21) + 1, 0, 0, 0, 0, p, p) == (-1, -1)
        for flags in (1, 3, 4, 8, -1):
            assert batch(p, p, p, 1, 2, 1, 1, flags, p, p) == (-1, -1), flags
        for hole in (0, 2, 3, 4):                    # setup, coeffs, out_proof, out_inf; the setup's flags alone may be null
            args = [p] * 5
            args[hole] = None
            assert batch(args[0], args[1], args[2], 1, 2, 1, 1, 0, args[3], args[4]) == (-1, -1), hole
        assert lib.zkp_kzg_cells_batch(None, p, p, p, 1, 2, 1, 1, 0, p, p) == -1
        assert batch(None, None, None, 0, 19, 19, 1, 2, None, None) == (0, 0)
        stp = lambda *a: (lib.zkp_kzg_cells_setup(h, *a), lib.zkp_kzg_cells_setup_dev(h, *a, None))
        assert stp(p, 20, 0, p, p) == (-1, -1) and stp(p, 2, 3, p, p) == (-1, -1)
        for hole in range(3):
            args = [p] * 3
            args[hole] = None
            assert stp(args[0], 2, 1, args[1], args[2]) == (-1, -1), hole
        ok = ctypes.c_int(7)
        okp = ctypes.cast(ctypes.byref(ok), ctypes.c_void_p)
        ver = lambda *a: (lib.zkp_kzg_cell_verify_batch(h, *a), lib.zkp_kzg_cell_verify_batch_dev(h, *a, None))
        full = [p, p, p, p, p, p, p, p, p]
        assert ver(*full, 1, 21, 1, 0, p, okp) == (-1, -1) and ver(*full, 1, 3, 4, 0, p, okp) == (-1, -1) and ver(*full, 1, 20, 16, 0, p, okp) == (-1, -1)
        assert ver(*full, (1 << 21) + 1, 3, 1, 0, p, okp) == (-1, -1) and ver(*full, 1, 3, 1, 1, p, okp) == (-1, -1) and ver(*full, 1, 3, 1, 16, p, okp) == (-1, -1)
        for hole in (0, 1, 2, 3, 5, 6, 7):           # the two arrays of flags alone may be null
            args = list(full)
            args[hole] = None
            assert ver(*args, 1, 3, 1, 0, p, okp) == (-1, -1), hole
        assert ver(*full, 1, 3, 1, 0, None, okp) == (-1, -1) and ver(*full, 1, 3, 1, 0, p, None) == (-1, -1)
        assert lib.zkp_kzg_cell_verify_batch(h, *([None] * 9), 0, 3, 1, 0, None, okp) == 0 and ok.value == 1
        with pytest.raises(ValueError):
            e.kzg_cells(setup[:7], sinf[:7], coeffs, log2_n, log2_l, 1)
    finally:
        e.close()


def test_plain_c_consumer_runs(tmp_path):
    """integration/c/zkp_cells.c: the header and the three calls from plain C (no Python, no torch types)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "zkvm_pairings_amd")
    exe = str(tmp_path / "zkp_cells")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "integration", "c", "zkp_cells.c"), "-L", libdir,
                           "-lzkp_pairings", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "zkp_cells ok" in out.stdout, out.stdout + out.stderr
