"""Call-order independence on one MI355X (run with -m gpu): every context owns grow-only workspaces that all call kinds share, so a
call that follows a larger one runs in a workspace full of the larger call's data.  Each test takes a FRESH engine (pytest's order and
-k cannot change what is exercised), runs a fixed sequence of sizes - large, 1, large, small, 65, 1 - on it, alternating resident
tensors and host arrays (the host slots and the `_dev` workspaces are different buffers of the same context), and checks EVERY answer
against the references of tests/replay_cases.py (Python integers, the construction of the inputs, the CPU oracle).  Above the oracle's
practical size (4097 pairings) the reference is the host flavour of a second, fresh engine whose first call it is, with a sample
of the values checked against the oracle."""
import random

import numpy as np
import pytest

import oracle_lib as o
import replay_cases as rc

pytestmark = pytest.mark.gpu
SEED = 0x0DE2
LARGE, SMALL = 4097, 5
FLAVOURS = ("dev", "host", "host", "dev", "host", "dev")        # large on either flavour, 1 on either flavour


@pytest.fixture(scope="module")
def helper():
    """makes the inputs (host-pointer scalar multiplications); never the engine under test"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def fresh():
    from zkvm_pairings_amd import PairingEngine
    return PairingEngine(0)


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def same(outs, want, what):
    if not isinstance(outs, tuple):
        outs = (outs,)
    assert len(outs) == len(want), what
    for i, (g, w) in enumerate(zip(outs, want)):
        if isinstance(g, (bool, int)):
            assert w.size == 1 and int(g) == int(w.reshape(-1)[0]), "%s: output %d is %r" % (what, i, g)
            continue
        got = g.cpu().numpy() if hasattr(g, "cpu") else np.ascontiguousarray(g)
        assert got.nbytes == w.nbytes, (what, i, got.shape, w.shape)
        assert got.tobytes() == np.ascontiguousarray(w).tobytes(), "%s: output %d differs" % (what, i)


def call(eng, case, shape, host, want, flavour, what):
    import torch
    if flavour == "dev":
        outs = case.run(eng, {x: to_dev(a) for x, a in host.items()}, shape)
        torch.cuda.synchronize()
    else:
        outs = case.run_host(eng, host, shape)
    same(outs, want, "%s %s (%s)" % (what, shape, flavour))


def case_of(id):
    return [c for c in rc.CASES if c.id == id][0]


def sequence(eng, helper, case, shapes):
    """step i runs set i mod 3 (A, B, C: other values, other verdicts, other flags) of inputs of its own"""
    for i, (shape, fl) in enumerate(zip(shapes, FLAVOURS)):
        sets, want = case.make(helper, shape, SEED + i)
        call(eng, case, shape, sets[i % 3], want[i % 3], fl, "%s step %d" % (case.id, i))


# ------------------------------------------------------------------------------------------------------------------- sizes large, 1, large, small, 65, 1
def test_pairing_sizes(helper):
    case = case_of("pairing-n65-k1")
    eng, ref = fresh(), fresh()
    try:
        for i, (n, fl) in enumerate(zip((LARGE, 1, LARGE, SMALL, 65, 1), FLAVOURS)):
            rng = random.Random(SEED + 100 + i)
            g1, g2 = rc._g1(helper, [rng.randrange(1, rc.R) for _ in range(n)]), rc._g2(helper, [rng.randrange(1, rc.R) for _ in range(n)])
            i1, i2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
            i1[(i + 2)::9] = 1
            i2[(2 * i + 5)::13] = 1
            if n <= 65:
                want = o.pairing_batch(g1, g2, i1, i2, nthreads=16)
            else:
                want = ref.pairing(g1, g2, i1, i2)                  # the host flavour on an engine that has seen no smaller or other call
                idx = np.array([0, 2, 5, n // 2, n - 2, n - 1])
                assert np.array_equal(want[idx], o.pairing_batch(g1[idx], g2[idx], i1[idx], i2[idx], nthreads=16))
                assert (want[(i1 | i2) != 0] == o.fp12_one()[None]).all()                # a flagged pair contributes one
            call(eng, case, (n, 1), dict(g1=g1, g2=g2, inf1=i1, inf2=i2), (want,), fl, "pairing step %d" % i)
    finally:
        eng.close()
        ref.close()


def test_pairing_check_k3_sizes(helper):
    """the verdicts are known by construction: the pairs of a good check cancel (sum x_j y_j = 0), a bad one is off by one"""
    case = case_of("pairing_check-n5-k3")
    eng = fresh()
    try:
        for i, (n, fl) in enumerate(zip((LARGE, 1, LARGE, SMALL, 65, 1), FLAVOURS)):
            rng = random.Random(SEED + 200 + i)
            bad = set(range(i % 3, n, 3 + i)) if i % 2 == 0 else ({n - 1} if i == 3 else set())
            g1, g2, i1 = rc.free_checks(helper, rng, n, 3, bad=bad, zero_first=(i % 2 == 1))
            ok = np.array([0 if c in bad else 1 for c in range(n)], dtype=np.uint8)
            host = dict(g1=g1, g2=g2, inf1=i1, inf2=np.zeros(3 * n, dtype=np.uint8))
            call(eng, case, (n, 3), host, (ok, rc._i32(ok.all())), fl, "pairing_check step %d" % i)
    finally:
        eng.close()


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("shared", [False, True])
def test_msm_sizes(helper, which, shared):
    case = case_of("g%d_msm-m65-x2%s" % (which, "-shared" if shared else ""))
    eng = fresh()
    try:
        sequence(eng, helper, case, [(m, 2, shared) for m in (LARGE, 1, LARGE, SMALL, 65, 1)])
    finally:
        eng.close()


def test_fr_fold_sizes(helper):
    eng = fresh()
    try:
        sequence(eng, helper, case_of("fr_fold-n65-l3"), [(n, 3) for n in (LARGE, 1, LARGE, SMALL, 65, 1)])
    finally:
        eng.close()


def test_fr_invert_sizes(helper):
    eng = fresh()
    try:
        sequence(eng, helper, case_of("fr_invert-n5"), [(n,) for n in (LARGE, 1, LARGE, SMALL, 65, 1)])
    finally:
        eng.close()


@pytest.mark.parametrize("compressed", [False, True])
def test_points_check_sizes(helper, compressed):
    eng = fresh()
    try:
        sequence(eng, helper, case_of("points_check%s-n321-k1" % ("_compressed" if compressed else "")),
                 [(n, 1) for n in (LARGE, 1, LARGE, SMALL, 65, 1)])
    finally:
        eng.close()


def test_kzg_sizes(helper):
    eng = fresh()
    try:
        sequence(eng, helper, case_of("kzg-n5"), [(n,) for n in (127, 1, 127, SMALL, 65, 1)])
    finally:
        eng.close()


def test_groth16_sizes(helper):
    eng = fresh()
    try:
        sequence(eng, helper, case_of("groth16-n5-l3"), [(127, 64), (1, 3), (127, 64), (5, 3), (65, 3), (1, 3)])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------- the cached domain table
@pytest.mark.parametrize("order", [(12, 6, 0, 9, 12), (0, 6, 12)], ids=["strided-reads-of-a-larger-table", "the-table-is-rebuilt-twice"])
def test_fr_eval_domain_table_sequences(helper, order):
    """12, 6, 0, 9, 12: after the first call the smaller domains are strided reads of the 2^12 table; 0, 6, 12: the table is rebuilt
    twice.  With and without bit-reversed order, both flavours, every answer equal to synthetic.barycentric_eval on Python integers."""
    eng = fresh()
    try:
        step = 0
        for lg in order:
            for bitrev in (False, True):
                sets, want = rc.eval_sets(lg, 2, bitrev, SEED + step)
                case = case_of("fr_eval-log9-x3-bitrev" if bitrev else "fr_eval-log9-x3")
                call(eng, case, (lg, 2, bitrev), sets[step % 3], want[step % 3], ("dev", "host")[(step // 2 + step) % 2], "fr_eval step %d" % step)
                step += 1
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------- mixed kinds on one context
def test_mixed_kinds_share_the_workspaces_in_either_order(helper):
    """KZG(127), g2_msm(65, 2, shared), Groth16(5, 3), RLC(24), g1_msm(1, 1), KZG(5), pairing(1) share msm_ws and the pairing
    workspace: each step gives its known answer, and the same seven calls in reverse order on a second fresh engine give the same"""
    plan = [("kzg-n5", (127,), 1), ("g2_msm-m65-x2-shared", (65, 2, True), 0), ("groth16-n5-l3", (5, 3), 2), ("rlc-groth-n24", (24,), 1),
            ("g1_msm-m1-x1", (1, 1, False), 2), ("kzg-n5", (5,), 0), ("pairing-n1-k1", (1, 1), 2)]
    steps = []
    for i, (id, shape, s) in enumerate(plan):
        case = case_of(id)
        sets, want = case.make(helper, shape, SEED + 300 + i)
        steps.append((case, shape, sets[s], want[s], ("dev", "host")[i % 2]))
    for name, order in (("forward", steps), ("reverse", steps[::-1])):
        eng = fresh()
        try:
            for case, shape, host, want, fl in order:
                call(eng, case, shape, host, want, fl, "mixed %s: %s" % (name, case.id))
        finally:
            eng.close()
