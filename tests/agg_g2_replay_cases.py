"""The device-pointer entry points of include/zkp_bls_agg_g2.h (helper of test_gpu_agg_g2_replay.py, test_gpu_call_order_agg_g2.py and
test_agg_g2_cpu.py; not a test module): the Case rows in the form of tests/replay_cases.py.  Expected values never come from the library
under test: sums, keys and signatures are made by tests/agg_g2_model.py on Python integers."""
import random

import numpy as np

import agg_g2_model as a2
import agg_model as am
import bls_replay_cases as brc
from agg_replay_cases import _cut
from replay_cases import Case

# every zkp_*_dev( of include/zkp_bls_agg_g2.h has a row below or a written reason here
EXCLUDED = {}

N_TABLE = 37


def _sum_sets(n_seg, n_idx, seed):
    """the three sets have one shape and different cuts, rows and signs; B holds a row beyond the table (status 1), C a cancelling pair"""
    pts = a2.g2_table(N_TABLE)
    rows = a2.g2_rows(pts)[0]
    sets, want = [], []
    for s in range(3):
        rng = random.Random(seed * 103 + s)
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
        sets.append(dict(table=rows, idx=a_idx.view(np.int32), seg_off=a_off))
        want.append(a2.sum_rows(pts, idx, seg_off))
    return sets, want


def _minsig_dst():
    return np.frombuffer(a2.MINSIG_DST, dtype=np.uint8).copy()


def _committee_sets(n, n_idx, seed):
    """A and C hold; B has one member of the longest committee replaced.  Committee sizes are fixed by (n, n_idx)"""
    _, pks = a2.minsig_key_table(N_TABLE)
    rows = a2.g2_rows(pks)[0]
    sizes = [n_idx - 2 * (n - 1)] + [2] * (n - 1)
    sets, want = [], []
    for s in range(3):
        b = a2.minsig_aggregate_batch(n, N_TABLE, seed + s, sizes=sizes)
        committees = [list(c) for c in b["committees"]]
        ok = 1
        if s == 1:
            committees[0][1] = next(r for r in range(N_TABLE) if r not in committees[0])
            ok = 0
        idx, seg_off = am.committee_entries(committees)
        a_idx, a_off = am.entry_arrays(idx, seg_off)
        buf, off = brc.pack(b["msgs"])
        pad = np.zeros(64 * n, dtype=np.uint8)                           # the longest of MESSAGES has 64 bytes
        pad[:buf.size] = buf
        sets.append(dict(table=rows, idx=a_idx.view(np.int32), seg_off=a_off, msgs=pad, offsets=off, dst=_minsig_dst(), sig=b["sig"],
                         rand=am.rand_rows(n, seed + 5 * s)))
        want.append((np.array([ok], dtype=np.int32),))
    return sets, want


def _aggv_sets(n, n_msg, seed):
    """A and C hold; in B two signatures change places (distinct rand rows: the batch fails).  The cuts differ between the sets"""
    sets, want = [], []
    for s in range(3):
        rng = random.Random(seed * 107 + s)
        sizes = [1 + k for k in _cut(n, n_msg - n, rng)]                  # no empty segment, none above 8
        while max(sizes) > 8:
            sizes = [1 + k for k in _cut(n, n_msg - n, rng)]
        b = a2.aggregate_verify_batch(sizes, seed=seed + s)
        sig, ok = b["sig"], 1
        if s == 1:
            sig = sig.copy()
            sig[[0, n - 1]] = sig[[n - 1, 0]]
            ok = 0 if n > 1 else 1
        buf, off = brc.pack(b["msgs"])
        pad = np.zeros(64 * n_msg, dtype=np.uint8)
        pad[:buf.size] = buf
        sets.append(dict(pk=b["pk"], msgs=pad, offsets=off, seg_off=np.array(b["seg_off"], dtype=np.uint64), dst=brc._dst_arr(), sig=sig,
                         rand=am.rand_rows(n, seed + 7 * s)))
        want.append((np.array([ok], dtype=np.int32),))
    return sets, want


# the smallest shapes that take two accumulation levels: more than msm::RUN = 32 entries; AggregateVerify: (signatures, messages)
CASES = [
    Case("g2_segment_sum-seg5-idx40", ["zkp_g2_segment_sum_batch_dev"], "g2_segment_sum", lambda hh, shape, seed: _sum_sets(shape[0], shape[1], seed),
         lambda e, t, sh: e.g2_segment_sum(t["table"], t["idx"], t["seg_off"]), (5, 40), (2, 5)),
    Case("bls_minsig_fast_aggregate_verify-n3-idx40", ["zkp_bls_minsig_fast_aggregate_verify_batch_dev"], "bls_minsig_fast_aggregate_verify",
         lambda hh, shape, seed: _committee_sets(shape[0], shape[1], seed),
         lambda e, t, sh: (e.bls_minsig_fast_aggregate_verify(t["table"], t["idx"], t["seg_off"], t["msgs"], t["sig"], t["dst"], offsets=t["offsets"],
                                                              rand=t["rand"]),),
         (3, 40), (2, 6)),
    Case("bls_aggregate_verify-n3-msg9", ["zkp_bls_aggregate_verify_batch_dev"], "bls_aggregate_verify",
         lambda hh, shape, seed: _aggv_sets(shape[0], shape[1], seed),
         lambda e, t, sh: (e.bls_aggregate_verify(t["pk"], t["msgs"], t["seg_off"], t["sig"], t["dst"], offsets=t["offsets"], rand=t["rand"]),),
         (3, 9), (2, 3)),
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
