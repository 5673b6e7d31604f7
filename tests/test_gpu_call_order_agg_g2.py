"""g2_segment_sum, bls_minsig_fast_aggregate_verify and bls_aggregate_verify between the calls whose workspace they share - g1_segment_sum
and bls_fast_aggregate_verify (ONE aggregation workspace holds the layouts of all five) - and the verifiers they drive, on ONE fresh
context, forward and reversed, with a large call, a call of one entry, a large and a small one: the workspace grows after another layout
has used it, and a small call runs inside a workspace that has stopped growing.  Every answer must be what the call gives alone.  Run
with -m gpu."""
import random

import numpy as np
import pytest

import agg_g2_model as a2
import agg_model as am
import bls_replay_cases as brc
from test_gpu_call_order_agg import _sum_case as _g1_sum_case
from test_gpu_call_order_agg import _verify_case as _g1_verify_case

pytestmark = pytest.mark.gpu
N_TABLE = 64


def _sum_case(eng, lens, seed):
    pts = a2.g2_table(N_TABLE)
    rows = a2.g2_rows(pts)[0]
    rng = random.Random(seed)
    idx = [rng.randrange(N_TABLE) | (am.SIGN if rng.randrange(4) == 0 else 0) for _ in range(sum(lens))]
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    want = a2.sum_rows(pts, idx, off)
    a_idx, a_off = am.entry_arrays(idx, off)
    return lambda: all(g.tobytes() == w.tobytes() for g, w in zip(eng.g2_segment_sum(rows, a_idx, a_off), want))


def _committee_case(eng, n, sizes, forged):
    import zkvm_pairings_amd as z
    _, pks = a2.minsig_key_table(N_TABLE)
    rows = a2.g2_rows(pks)[0]
    b = a2.minsig_aggregate_batch(n, N_TABLE, 3, sizes=sizes)
    committees = [list(c) for c in b["committees"]]
    if forged:
        committees[n - 1][0] = next(r for r in range(N_TABLE) if r not in committees[n - 1])
    return lambda: z.bls_minsig_fast_aggregate_verify_batch(rows, committees, b["msgs"], b["sig"], a2.MINSIG_DST, rand=am.rand_rows(n, 9),
                                                            engine=eng) is not forged


def _aggv_case(eng, sizes, forged):
    import zkvm_pairings_amd as z
    b = a2.aggregate_verify_batch(sizes, seed=3)
    msgs = list(b["msgs"])
    if forged:
        msgs[-1] = b"not what was signed"
    off = np.array(b["seg_off"], dtype=np.uint64)
    return lambda: z.bls_aggregate_verify_batch(b["pk"], msgs, off, b["sig"], brc.DST, rand=am.rand_rows(len(sizes), 9), engine=eng) is not forged


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_g1_and_g2_aggregation_calls_share_one_workspace(order):
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)                           # a fresh context per order: every workspace starts empty
    try:
        big, sizes = (300, 0, 45, 1), [40, 2, 1, 33, 7, 12]
        steps = [_sum_case(eng, big, 1), _g1_sum_case(eng, (1,), 2), _aggv_case(eng, [3, 7, 1, 2, 5, 8, 8], False), _sum_case(eng, (1,), 3),
                 _g1_verify_case(eng, 6, sizes, False), _committee_case(eng, 6, sizes, False), _aggv_case(eng, [1], False), _g1_sum_case(eng, big, 4),
                 _committee_case(eng, 1, [1], False), _sum_case(eng, big, 5), _aggv_case(eng, [3, 7, 1, 2, 5, 8, 8], True), _g1_verify_case(eng, 2, [3, 2], False),
                 _committee_case(eng, 6, sizes, True), _sum_case(eng, (2, 3), 6), _aggv_case(eng, [2, 1], False), _committee_case(eng, 2, [3, 2], False),
                 _g1_verify_case(eng, 6, sizes, True)]
        if order == "reversed":
            steps = steps[::-1]
        for i, step in enumerate(steps):
            assert step(), (order, i)
    finally:
        eng.close()
