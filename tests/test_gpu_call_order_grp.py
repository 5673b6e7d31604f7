"""g1_scaled_segment_sum, bls_verify_grouped and bls_fast_aggregate_verify_grouped between the calls whose workspaces they share -
bls_verify (the hash's workspace, the MSM's, the Fp12 records), g1_segment_sum (the aggregate form sums into its workspace) and hash_to_g2
- on ONE fresh context, forward and reversed, with a large call, a call of one signature, a large and a small one: each workspace grows
after another call has used it, and a small call runs inside a workspace that has stopped growing.  Every answer must be what the call
gives alone.  Run with -m gpu."""
import random

import numpy as np
import pytest

import agg_model as am
import bls_replay_cases as brc
import grp_model as gm
import h2c_model as h

pytestmark = pytest.mark.gpu
N_KEYS = 36


def _scaled_case(eng, lens, seed):
    sks, pks = am.key_table(N_KEYS)
    rows = am.table_rows(pks)
    rng = random.Random(seed)
    picks = [rng.randrange(N_KEYS) for _ in range(sum(lens))]
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    rand = gm.rand_rows(len(picks), seed)
    want = gm.sum_rows([sks[r] for r in picks], gm.rand_pairs(rand), off)
    return lambda: all(g.tobytes() == w.tobytes() for g, w in zip(eng.g1_scaled_segment_sum(rows[picks], rand, gm.off_array(off)), want))


def _segment_case(eng, lens, seed):
    _, pks = am.key_table(gm.N_TABLE)
    rows = am.table_rows(pks)
    rng = random.Random(seed)
    idx = [rng.randrange(gm.N_TABLE) | (am.SIGN if rng.randrange(4) == 0 else 0) for _ in range(sum(lens))]
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    want = am.sum_rows(pks, idx, off)
    a_idx, a_off = am.entry_arrays(idx, off)
    return lambda: all(g.tobytes() == w.tobytes() for g, w in zip(eng.g1_segment_sum(rows, a_idx, a_off), want))


def _grouped_case(eng, sizes, forged):
    b = gm.grouped_batch(sizes, 3)
    sig = b["sig"]
    if forged:
        sig = sig.copy()
        sig[[0, 1]] = sig[[1, 0]]
    n = sig.shape[0]
    return lambda: eng.bls_verify_grouped(b["pk"], gm.off_array(b["grp_off"]), b["msgs"], sig, brc.DST, rand=gm.rand_rows(n, 9)) is not forged


def _aggregate_case(eng, sizes, groups, forged):
    import zkvm_pairings_amd as z
    sks, pks = am.key_table(gm.N_TABLE)
    rows = am.table_rows(pks)
    b = am.aggregate_batch(len(sizes), gm.N_TABLE, 5, sizes=sizes)
    expanded = [am.MESSAGES[g] for g, k in enumerate(groups) for _ in range(k)]
    sig = am.u64([h.g2_words(am.sign(x, sum(sks[r] for r in c)))[0] for x, c in zip(expanded, b["committees"])]).reshape(-1, 24)
    committees = [list(c) for c in b["committees"]]
    if forged:
        committees[-1][0] = next(r for r in range(gm.N_TABLE) if r not in committees[-1])
    return lambda: z.bls_fast_aggregate_verify_grouped_batch(rows, committees, expanded, sig, brc.DST, rand=gm.rand_rows(len(sizes), 9), engine=eng) is not forged


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_grouped_calls_between_bls_verify_segment_sums_and_hash(order):
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)                                # a fresh context: every workspace starts empty
    try:
        small = brc.batch(5, 3)
        few = [b"", b"one", bytes(range(56))]
        want, winf = brc.point_rows([brc.hashed(x, brc.DST) for x in few])
        bls = lambda: z.bls_verify_batch(small["pk"], small["msgs"], small["sig"], brc.DST, rand=brc.rand_rows(5, 9), engine=eng) is True

        def hashes():
            pts, inf = eng.hash_to_g2(few, brc.DST)
            return pts.tobytes() == want.tobytes() and inf.tobytes() == winf.tobytes()
        large, large_agg = [1, 33, 0, 32, 4], ([40, 2, 1, 33, 7, 12], [3, 0, 2, 1])
        steps = [_grouped_case(eng, large, False), bls, _grouped_case(eng, [1], False), _segment_case(eng, (300, 0, 45, 1), 1),
                 _scaled_case(eng, (300, 0, 45, 1), 1), hashes, _grouped_case(eng, large, True), _aggregate_case(eng, *large_agg, False), _scaled_case(eng, (1,), 2),
                 bls, _grouped_case(eng, [2, 3], False), _aggregate_case(eng, [1], [1], False), _segment_case(eng, (2, 3), 4),
                 _aggregate_case(eng, *large_agg, True), _scaled_case(eng, (2, 3), 4), _aggregate_case(eng, [3, 2], [1, 1], False), _grouped_case(eng, [2, 3], True)]
        if order == "reversed":
            steps = steps[::-1]
        for i, step in enumerate(steps):
            assert step(), (order, i)
    finally:
        eng.close()
