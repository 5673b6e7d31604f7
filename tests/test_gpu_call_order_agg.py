"""g1_segment_sum and bls_fast_aggregate_verify between the calls whose workspaces they share - bls_verify (the BLS and RLC workspaces the
verifier runs on), an MSM (whose accumulation kernel sums the segments) and hash_to_g2 - on ONE context, forward and reversed, with a
large call, a call of one entry, a large and a small one: each workspace grows after another call has used it, and a small call runs inside
a workspace that has stopped growing.  Every answer must be what the call gives alone.  Run with -m gpu."""
import random

import numpy as np
import pytest

import agg_model as am
import bls_replay_cases as brc
from test_gpu_call_order_bls import _msm_case

pytestmark = pytest.mark.gpu
N_TABLE = 64


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def _sum_case(eng, lens, seed):
    _, pks = am.key_table(N_TABLE)
    rows = am.table_rows(pks)
    rng = random.Random(seed)
    idx = [rng.randrange(N_TABLE) | (am.SIGN if rng.randrange(4) == 0 else 0) for _ in range(sum(lens))]
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    want = am.sum_rows(pks, idx, off)
    a_idx, a_off = am.entry_arrays(idx, off)
    return lambda: all(g.tobytes() == w.tobytes() for g, w in zip(eng.g1_segment_sum(rows, a_idx, a_off), want))


def _verify_case(eng, n, sizes, forged):
    import zkvm_pairings_amd as z
    _, pks = am.key_table(N_TABLE)
    rows = am.table_rows(pks)
    b = am.aggregate_batch(n, N_TABLE, 3, sizes=sizes)
    committees = [list(c) for c in b["committees"]]
    if forged:
        committees[n - 1][0] = next(r for r in range(N_TABLE) if r not in committees[n - 1])
    return lambda: z.bls_fast_aggregate_verify_batch(rows, committees, b["msgs"], b["sig"], brc.DST, rand=am.rand_rows(n, 9), engine=eng) is not forged


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_aggregation_calls_between_bls_verify_msm_and_hash(eng, order):
    import zkvm_pairings_amd as z
    small = brc.batch(5, 3)
    few = [b"", b"one", bytes(range(56))]
    want, winf = brc.point_rows([brc.hashed(x, brc.DST) for x in few])
    bls = lambda: z.bls_verify_batch(small["pk"], small["msgs"], small["sig"], brc.DST, rand=brc.rand_rows(5, 9), engine=eng) is True

    def hashes():
        pts, inf = eng.hash_to_g2(few, brc.DST)
        return pts.tobytes() == want.tobytes() and inf.tobytes() == winf.tobytes()
    steps = [_sum_case(eng, (300, 0, 45, 1), 1), bls, _sum_case(eng, (1,), 2), _msm_case(eng, 70), _verify_case(eng, 6, [40, 2, 1, 33, 7, 12], False), hashes,
             _verify_case(eng, 1, [1], False), bls, _sum_case(eng, (300, 0, 45, 1), 3), _msm_case(eng, 9), _verify_case(eng, 6, [40, 2, 1, 33, 7, 12], True),
             _sum_case(eng, (2, 3), 4), _verify_case(eng, 2, [3, 2], False)]
    if order == "reversed":
        steps = steps[::-1]
    for i, step in enumerate(steps):
        assert step(), (order, i)
