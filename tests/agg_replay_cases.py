"""The device-pointer entry points of include/zkp_bls_agg.h (helper of test_gpu_agg_replay.py, test_gpu_call_order_agg.py and
test_agg_cpu.py; not a test module): the Case rows in the form of tests/replay_cases.py.  Expected values never come from the library
under test: sums, keys and signatures are made by tests/agg_model.py on Python integers."""
import random

import numpy as np

import agg_model as am
import bls_replay_cases as brc
from replay_cases import Case

# every zkp_*_dev( of include/zkp_bls_agg.h has a row below or a written reason here
EXCLUDED = {}

N_TABLE = 37


def _cut(n_seg, n_idx, rng):
    """n_seg segment lengths that add up to n_idx, some of them empty"""
    cuts = sorted(rng.randrange(n_idx + 1) for _ in range(n_seg - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [n_idx])]


def _sum_sets(n_seg, n_idx, seed):
    """the three sets have one shape and different cuts, rows and signs; B holds a row beyond the table (status 1), C a cancelling pair"""
    _, pks = am.key_table(N_TABLE)
    sets, want = [], []
    for s in range(3):
        rng = random.Random(seed * 101 + s)
        lens = _cut(n_seg, n_idx, rng)
        idx = [rng.randrange(N_TABLE) | (am.SIGN if rng.randrange(4) == 0 else 0) for _ in range(n_idx)]
        seg_off = [0]
        for k in lens:
            seg_off.append(seg_off[-1] + k)
        if s == 1:
            idx[n_idx // 2] = N_TABLE
        if s == 2 and n_idx >= 2:
            idx[1] = idx[0] ^ am.SIGN
        a_idx, a_off = am.entry_arrays(idx, seg_off)
        sets.append(dict(table=am.table_rows(pks), idx=a_idx.view(np.int32), seg_off=a_off))
        want.append(am.sum_rows(pks, idx, seg_off))
    return sets, want


def _verify_sets(n, n_idx, seed):
    """A and C hold; B has one member of the longest committee replaced.  Committee sizes are fixed by (n, n_idx), so the buffers keep
    their shape; the members and messages change"""
    _, pks = am.key_table(N_TABLE)
    sizes = [n_idx - 2 * (n - 1)] + [2] * (n - 1)
    sets, want = [], []
    for s in range(3):
        b = am.aggregate_batch(n, N_TABLE, seed + s, sizes=sizes)
        committees = [list(c) for c in b["committees"]]
        ok = 1
        if s == 1:
            committees[0][3] = next(r for r in range(N_TABLE) if r not in committees[0])
            ok = 0
        idx, seg_off = am.committee_entries(committees)
        a_idx, a_off = am.entry_arrays(idx, seg_off)
        buf, off = brc.pack(b["msgs"])
        pad = np.zeros(64 * n, dtype=np.uint8)                           # the longest of MESSAGES has 64 bytes
        pad[:buf.size] = buf
        sets.append(dict(table=am.table_rows(pks), idx=a_idx.view(np.int32), seg_off=a_off, msgs=pad, offsets=off, dst=brc._dst_arr(), sig=b["sig"],
                         rand=am.rand_rows(n, seed + 5 * s)))
        want.append((np.array([ok], dtype=np.int32),))
    return sets, want


# the smallest shapes that take two accumulation levels: more than msm::RUN = 32 entries
CASES = [
    Case("g1_segment_sum-seg5-idx40", ["zkp_g1_segment_sum_batch_dev"], "g1_segment_sum", lambda hh, shape, seed: _sum_sets(shape[0], shape[1], seed),
         lambda e, t, sh: e.g1_segment_sum(t["table"], t["idx"], t["seg_off"]), (5, 40), (2, 5)),
    Case("bls_fast_aggregate_verify-n3-idx40", ["zkp_bls_fast_aggregate_verify_batch_dev"], "bls_fast_aggregate_verify",
         lambda hh, shape, seed: _verify_sets(shape[0], shape[1], seed),
         lambda e, t, sh: (e.bls_fast_aggregate_verify(t["table"], t["idx"], t["seg_off"], t["msgs"], t["sig"], t["dst"], offsets=t["offsets"], rand=t["rand"]),),
         (3, 40), (2, 6)),
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
