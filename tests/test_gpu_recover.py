"""The cell recovery on one MI355X (zkp_das_recover_batch, include/zkp_recover.h), byte for byte: a consistent blob comes back as the
polynomial its cells were made from (tests/recover_replay_cases.py: cells by poly_model's transform, nothing from the library under
test), a blob with too few cells as zeros, a corrupted blob with exactly M / 2 cells as tests/recover_model.py's interpolant.  The shapes
are the smallest that reach each path of k_rec_column and of its driver (tests/recover_shapes.py); every erasure pattern and every
corruption case on the 16, 4 shape; validation mode; a slice boundary; host against device flavour; the argument errors; the round trip
through the cell producer and the cell verifier at PeerDAS shape; the plain C consumer.  Run with -m gpu."""
import ctypes
import random

import numpy as np
import pytest

import cells_model as cm
import cells_replay_cases as crc
import poly_model as pm
import recover_model as rm
import recover_replay_cases as rrc
import recover_shapes as rs
import slice_pools as sp
from replay_cases import fr_rows

pytestmark = pytest.mark.gpu
R = pm.R
KINDS_BY_N = {1: ("random-half",), 2: ("random-half", "even"), 3: ("random-half", "one", "few"), 5: ("first-half", "odd", "few", "none", "half-bad")}


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


def from_dev(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def both_flavours(eng, inst, log2_n, log2_l, bitrev, what):
    co, ok = eng.das_recover(inst["values"], inst["present"], log2_n, log2_l, bitrev)
    rrc.check(co, ok, inst, what + " host")
    dco, dok = eng.das_recover(to_dev(inst["values"]), to_dev(inst["present"]), log2_n, log2_l, bitrev)
    rrc.check(from_dev(dco), from_dev(dok), inst, what + " dev")
    # host against device flavour: the same bytes, the unspecified rows included (the arithmetic is exact)
    assert from_dev(dco).tobytes() == co.tobytes() and from_dev(dok).tobytes() == ok.tobytes(), what
    return co, ok


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("shape", rs.GPU_SHAPES, ids=["N%d-l%d" % (1 << s[0], 1 << s[1]) for s in rs.GPU_SHAPES])
def test_every_path_of_the_table(eng, shape, bitrev):
    log2_n, log2_l, n, _ = shape
    inst = rrc.instance(KINDS_BY_N[n], log2_n, log2_l, bitrev, 0x5E0 + n)
    both_flavours(eng, inst, log2_n, log2_l, bitrev, "N=2^%d l=2^%d" % (log2_n, log2_l))


@pytest.mark.parametrize("bitrev", [False, True])
def test_every_erasure_pattern(eng, bitrev):
    inst = rrc.instance(rm.PATTERNS, *rs.SMALL, bitrev, 0x9A7)
    assert inst["ok"].all() and not inst["free"]
    both_flavours(eng, inst, *rs.SMALL, bitrev, "patterns")


@pytest.mark.parametrize("bitrev", [False, True])
def test_corrupted_and_missing_blobs_between_good_ones(eng, bitrev):
    """more than M / 2 cells with a corrupted value: ok = 0; exactly M / 2: ok = 1 and the other interpolant; M / 2 - 1: ok = 0 and a zero
    row - each between blobs that recover, whose rows and flags stay right"""
    kinds = ("random-half", "more-bad", "one", "half-bad", "even", "few", "none")
    inst = rrc.instance(kinds, *rs.SMALL, bitrev, 0xBAD)
    assert inst["ok"].tolist() == [1, 0, 1, 1, 1, 0, 1] and inst["free"] == [1]
    co, ok = both_flavours(eng, inst, *rs.SMALL, bitrev, "corruption")
    n_co = 1 << rs.SMALL[0]
    assert not co.reshape(len(kinds), -1)[5].any() and co.reshape(len(kinds), n_co, 4)[3].tobytes() == inst["coeffs"].reshape(len(kinds), n_co, 4)[3].tobytes()


def test_validation_mode_looks_at_present_cells_only():
    from zkvm_pairings_amd import PairingEngine, ZkpError
    log2_n, log2_l = rs.SMALL
    l = 1 << log2_l
    inst = rrc.instance(("random-half", "even", "one"), log2_n, log2_l, True, 0x7A1)
    e = PairingEngine(0, validate=True)
    try:
        vals, pres = inst["values"].copy(), inst["present"]
        vals.reshape(-1, l, 4)[pres == 0] = np.uint64(0xFFFFFFFFFFFFFFFF)          # missing cells: 0xff bytes throughout
        co, ok = e.das_recover(vals, pres, log2_n, log2_l, True)                      # status OK, the output unchanged
        rrc.check(co, ok, inst, "0xff host")
        dco, dok = e.das_recover(to_dev(vals), to_dev(pres), log2_n, log2_l, True)
        rrc.check(from_dev(dco), from_dev(dok), inst, "0xff dev")
        assert e.take_validation_status() is False
        bad = vals.copy()
        cell = int(np.nonzero(pres)[0][-1])                                           # the last present cell of the batch, its last value
        bad.reshape(-1, l, 4)[cell, l - 1] = fr_rows([R])[0]                          # r itself: the smallest value that is not canonical
        with pytest.raises(ZkpError) as ei:
            e.das_recover(bad, pres, log2_n, log2_l, True)
        assert ei.value.status == -4
        e.das_recover(to_dev(bad), to_dev(pres), log2_n, log2_l, True)
        assert e.take_validation_status() is True and e.take_validation_status() is False
    finally:
        e.close()


@pytest.mark.parametrize("bitrev", [False, True])
def test_one_call_across_a_slice_boundary_with_a_short_last_slice(eng, bitrev):
    call = rrc.slice_call(bitrev)
    assert len(call.starts) == 2 and call.tail == 3                      # test_recover_cpu.py holds the slice length to the planner's
    for name in ("coeffs", "ok"):                                        # a build that computed slice 1 from offset 0 would not pass
        assert sp.reading(call, name, "zero").tobytes() != call.want(name).tobytes()
    co, ok = eng.das_recover(call.arg("values"), call.arg("present"), rs.SLICE_LOG2_N, rs.SLICE_LOG2_L, bitrev)
    assert sp.first_difference(ok, call.want("ok"), 1, call) is None
    assert sp.first_difference(co, call.want("coeffs"), 4, call) is None
    assert ok.tobytes() == call.want("ok").tobytes() and co.tobytes() == call.want("coeffs").tobytes()


def test_argument_errors_and_the_empty_call(eng):
    lib, h = eng._lib, eng._h
    buf = np.zeros((64, 4), dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    call = lambda *a: (lib.zkp_das_recover_batch(h, *a), lib.zkp_das_recover_batch_dev(h, *a, None))
    assert call(p, p, 1, 20, 10, 0, p, p) == (-1, -1)                    # log2_n > 19
    assert call(p, p, 1, 2, 3, 0, p, p) == (-1, -1)                      # log2_l > log2_n
    assert call(p, p, 1, 10, 0, 0, p, p) == (-1, -1)                     # M = 2048
    assert call(p, p, 1, 19, 9, 0, p, p) == (-1, -1)                     # M = 2048 at the largest N
    assert call(p, p, (1 << 23) + 1, 2, 1, 0, p, p) == (-1, -1)          # n D > 2^26
    assert call(p, p, 65, 19, 19, 0, p, p) == (-1, -1)
    for flags in (1, 3, 4, 8, -1):
        assert call(p, p, 1, 2, 1, flags, p, p) == (-1, -1), flags
    for hole in range(4):
        args = [p] * 4
        args[hole] = None
        assert call(args[0], args[1], 1, 2, 1, 0, args[2], args[3]) == (-1, -1), hole
    assert lib.zkp_das_recover_batch(None, p, p, 1, 2, 1, 0, p, p) == -1 and lib.zkp_das_recover_batch_dev(None, p, p, 1, 2, 1, 0, p, p, None) == -1
    assert call(None, None, 0, 19, 10, 2, None, None) == (0, 0)          # n == 0 is legal
    co, ok = eng.das_recover(np.zeros((0, 4), dtype=np.uint64), np.zeros(0, dtype=np.uint8), 4, 2, True)
    assert co.shape == (0, 4) and ok.shape == (0,)
    with pytest.raises(ValueError):
        eng.das_recover(buf[:7], np.ones(4, dtype=np.uint8), 2, 1)


def test_round_trip_recover_then_every_cell_verifies_at_peerdas_shape(eng, helper):
    """one blob of 4096 coefficients, 64 of its 128 cells: recover_cells_and_kzg_proofs_batch, then kzg_cell_verify_batch accepts all 128
    cells against the commitment of the ORIGINAL polynomial"""
    import zkvm_pairings_amd as z
    log2_n, log2_l = rs.PEERDAS
    big_m, l = 2 << (log2_n - log2_l), 1 << log2_l
    rng = random.Random(0xDA5)
    f = [rng.randrange(R) for _ in range(1 << log2_n)]
    cells = rm.cells_of(f, log2_n, log2_l, True)
    have = sorted(rng.sample(range(big_m), big_m // 2))
    from zkvm_pairings_amd import synthetic
    powers = [1] * (1 << log2_n)
    for i in range(1, len(powers)):
        powers[i] = powers[i - 1] * crc.TAU % R
    g1s, _ = helper.g1_mul(synthetic.G1_GENERATOR, fr_rows(powers + [cm.horner(f, crc.TAU)]))     # the setup and the commitment: not from the recovery
    mono_n, com = g1s[:-1].copy(), g1s[-1:].copy()
    setup = z.kzg_cells_setup(mono_n, log2_l, engine=helper)
    co, ok = z.recover_polynomials_batch([have], [fr_rows([v for m in have for v in cells[m]])], log2_n, log2_l, bitrev=True, engine=eng)
    assert ok.tolist() == [1] and co.tobytes() == fr_rows(f).tobytes()
    out_cells, proof, pinf, ok = z.recover_cells_and_kzg_proofs_batch(setup, [have], [fr_rows([v for m in have for v in cells[m]])], bitrev=True, engine=eng)
    assert ok.tolist() == [1] and out_cells.shape == (1, big_m, l, 4) and proof.shape == (1, big_m, 12)
    assert out_cells.tobytes() == fr_rows([v for row in cells for v in row]).tobytes()
    mono, g2, tg2 = mono_n[:l].copy(), crc.g2_generator(), crc.tau_l_g2_for(helper, log2_l)
    assert z.kzg_cell_verify_batch(mono, g2, tg2, np.repeat(com, big_m, axis=0), np.arange(big_m), out_cells[0], proof[0], log2_n + 1, bitrev=True, engine=eng,
                                   inf_proof=pinf[0]) is True
    with pytest.raises(ValueError):
        z.recover_polynomials_batch([[0, 0]], [out_cells[0, :2]], log2_n, log2_l, engine=eng)


def test_plain_c_consumer_runs(tmp_path):
    """integration/c/zkp_recover.c: recover, then the transform, then the cell proofs from plain C (no Python, no torch types)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "zkvm_pairings_amd")
    exe = str(tmp_path / "zkp_recover")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "integration", "c", "zkp_recover.c"), "-L", libdir,
                           "-lzkp_pairings", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "zkp_recover ok" in out.stdout, out.stdout + out.stderr
