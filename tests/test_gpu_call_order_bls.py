"""bls_verify between the calls whose workspaces it shares - the batch check by random linear combination and the MSM - on ONE context, in
both orders and with sizes that make each workspace grow after the other has used it: every answer must be what the call gives alone.
And sliced calls between small ones: the slice length of a call, and with it the stride of the point workspace, is min(n, 2^17), so it
changes from call to call inside a workspace that has stopped growing.  Run with -m gpu."""
import numpy as np
import pytest

import bls12_381_model as m
import bls_replay_cases as brc
import h2c_model as h

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def _rlc_case(eng, n):
    """n checks e(a_i g1, g2) e(-g1, a_i g2) == 1 as one free pair and one column with the fixed -g1"""
    from zkvm_pairings_amd import synthetic
    sc = synthetic.scalars(0xCA11 + n, n)
    g1, _ = eng.g1_mul(synthetic.G1_GENERATOR, sc)
    g2, _ = eng.g2_mul(synthetic.G2_GENERATOR, sc)
    neg = brc.u64(h.g1_words(m.g1_neg(m.G1_GEN))[0])
    return lambda: eng.pairing_check_rlc(g1, np.tile(synthetic.G2_GENERATOR, (n, 1)), 1, col_g2=g2, fixed_g1=neg, rand=brc.rand_rows(n, n))


def _msm_case(eng, n):
    from zkvm_pairings_amd import synthetic
    sc = synthetic.scalars(0x3535 + n, n)
    pts, _ = eng.g1_mul(synthetic.G1_GENERATOR, sc)
    ones = np.zeros((n, 4), dtype=np.uint64)
    ones[:, 0] = 1
    total = sum(synthetic.scalar_to_int(r) for r in sc) % h.R_ORDER
    want = brc.u64(h.g1_words(m.g1_mul(m.G1_GEN, total))[0])
    return lambda: eng.g1_msm(pts, ones)[0].tobytes() == want.tobytes()


@pytest.mark.parametrize("order", ["bls-first", "bls-last"])
def test_bls_verify_between_rlc_and_msm(eng, order):
    small, big = brc.batch(5, 3), brc.batch(61, 4)
    bad = dict(big, msgs=[b"x" + x for x in big["msgs"]])
    import zkvm_pairings_amd as z
    v = lambda b, want: z.bls_verify_batch(b["pk"], b["msgs"], b["sig"], brc.DST, rand=brc.rand_rows(len(b["msgs"]), 9), engine=eng) is want
    steps = [lambda: v(small, True), _rlc_case(eng, 40), _msm_case(eng, 70), lambda: v(big, True), _rlc_case(eng, 3), lambda: v(bad, False),
             _msm_case(eng, 9), lambda: v(small, True)]
    if order == "bls-last":
        steps = steps[1:3] + steps[:1] + steps[4:5] + steps[3:4] + steps[5:]
    for i, step in enumerate(steps):
        assert step(), (order, i)


def test_small_calls_between_sliced_ones_in_a_grown_workspace():
    """on a fresh context: hash_to_g2 on 2^17 + 61 messages (the workspace grows to its largest), on 1, sliced again, on 5; then bls_verify
    on 5 and on 2^17 + 6 signatures.  Every answer is checked against the model (tests/slice_pools.py assembles the large ones)"""
    import slice_pools as sp
    import test_gpu_slices as tgs
    from zkvm_pairings_amd import PairingEngine
    big, vbig = sp.hash_call(True), sp.verify_call()
    few = [b"", b"one", bytes(range(56)), b"\x00" * 64, bytes(range(119, 0, -1))]
    want, winf = brc.point_rows([brc.hashed(x, brc.DST) for x in few])
    small = brc.batch(5, 3)
    e = PairingEngine(0)
    try:
        def sliced(step):
            pts, inf = e.hash_to_g2(tgs.to_dev(big.msgs), brc.DST, offsets=tgs.to_dev(big.offsets))
            tgs.same(big, dict(points=pts, inf=inf), "hash_to_g2, step %d" % step)

        def short(k, step):
            pts, inf = e.hash_to_g2(few[:k], brc.DST)
            assert inf.tobytes() == winf[:k].tobytes() and pts.tobytes() == want[:k].tobytes(), step
        sliced(0)
        short(1, 1)
        sliced(2)
        short(5, 3)
        assert e.bls_verify(small["pk"], small["msgs"], small["sig"], brc.DST, rand=brc.rand_rows(5, 9)) is True, 4
        swapped = dict(small, sig=small["sig"][[1, 0, 2, 3, 4]])
        assert e.bls_verify(swapped["pk"], swapped["msgs"], swapped["sig"], brc.DST, rand=brc.rand_rows(5, 9)) is False, 4
        args = (vbig.arg("pk"), vbig.msgs, vbig.arg("sig"), brc.DST)
        assert e.bls_verify(*args, offsets=vbig.offsets, rand=vbig.arg("rand")) is True, 5
        bad = sp.forged_messages(vbig, vbig.forged[1])
        assert e.bls_verify(vbig.arg("pk"), bad, vbig.arg("sig"), brc.DST, offsets=vbig.offsets, rand=vbig.arg("rand")) is False, 5
        short(5, 6)
    finally:
        e.close()
