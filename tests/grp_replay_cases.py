"""The device-pointer entry points of include/zkp_bls_grouped.h (helper of test_gpu_grp_replay.py and test_grp_cpu.py; not a test
module): the Case rows in the form of tests/replay_cases.py.  Expected values never come from the library under test: sums, keys and
signatures are made by tests/grp_model.py and tests/agg_model.py on Python integers."""
import random

import numpy as np

import agg_model as am
import bls_replay_cases as brc
import grp_model as gm
import h2c_model as h
from replay_cases import Case

# every zkp_*_dev( of include/zkp_bls_grouped.h has a row below or a written reason here
EXCLUDED = {}

N_KEYS = 36


def _cut(n_seg, n, rng):
    """n_seg segment lengths that add up to n, some of them empty"""
    cuts = sorted(rng.randrange(n + 1) for _ in range(n_seg - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [n])]


def _offsets(lens):
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    return off


def _sum_sets(n_seg, n, seed):
    """the three sets have one shape and different cuts, points and scalars; B holds a zero scalar and an input at infinity, C a
    cancelling pair"""
    sks, pks = am.key_table(N_KEYS)
    rows = am.table_rows(pks)
    sets, want = [], []
    for s in range(3):
        rng = random.Random(seed * 101 + s)
        off = _offsets(_cut(n_seg, n, rng))
        picks = [rng.randrange(N_KEYS) for _ in range(n)]
        logs = [sks[r] for r in picks]
        pts, inf = rows[picks].copy(), np.zeros(n, dtype=np.uint8)
        rand = gm.rand_rows(n, seed * 7 + s)
        if s == 1:
            rand[n // 2] = 0
            pts[0], inf[0], logs[0] = am.g1_rows([None])[0][0], 1, None
        if s == 2 and n >= 2:
            logs[1] = gm.R - logs[0]
            pts[1] = am.g1_rows([am.public_key(logs[1])])[0][0]
            rand[1] = rand[0]
            off = [0, 2] + [max(2, v) for v in off[2:]] if n_seg > 1 else off        # both in segment 0
        sets.append(dict(pts=pts, inf=inf, rand=rand, seg_off=gm.off_array(off)))
        want.append(gm.sum_rows(logs, gm.rand_pairs(rand), off))
    return sets, want


def _batch_arrays(b, n, seed):
    buf, off = brc.pack(b["msgs"])
    pad = np.zeros(64 * len(b["msgs"]), dtype=np.uint8)                   # the longest of MESSAGES has 64 bytes
    pad[:buf.size] = buf
    return dict(msgs=pad, offsets=off, dst=brc._dst_arr(), rand=gm.rand_rows(n, seed))


def _verify_sets(m, n, seed):
    """A and C hold; B has two signatures of the longest group swapped.  Group sizes are fixed by (m, n): the buffers keep their shape,
    the signers change"""
    sizes = [n - 2 * (m - 1)] + [2] * (m - 1)
    sets, want = [], []
    for s in range(3):
        b = gm.grouped_batch(sizes, seed + s)
        sig, ok = b["sig"], 1
        if s == 1:
            sig = sig.copy()
            sig[[0, 1]] = sig[[1, 0]]
            ok = 0
        t = _batch_arrays(b, n, seed + 5 * s)
        t.update(pk=b["pk"], grp_off=gm.off_array(b["grp_off"]), sig=sig)
        sets.append(t)
        want.append((np.array([ok], dtype=np.int32),))
    return sets, want


def _aggregate_sets(m, n_idx, seed):
    """m messages, 2 m committees (two per message): the first committee holds n_idx - 2 (2 m - 1) members, the others two.  A and C hold;
    B has one member of the longest committee replaced"""
    sks, pks = am.key_table(gm.N_TABLE)
    n = 2 * m
    sizes = [n_idx - 2 * (n - 1)] + [2] * (n - 1)
    msgs = list(am.MESSAGES[:m])
    grp_off = [2 * g for g in range(m + 1)]
    sets, want = [], []
    for s in range(3):
        b = am.aggregate_batch(n, gm.N_TABLE, seed + s, sizes=sizes)
        sig = am.u64([h.g2_words(am.sign(msgs[i // 2], sum(sks[r] for r in c)))[0] for i, c in enumerate(b["committees"])]).reshape(-1, 24)
        committees = [list(c) for c in b["committees"]]
        ok = 1
        if s == 1:
            committees[0][0] = next(r for r in range(gm.N_TABLE) if r not in committees[0])
            ok = 0
        a_idx, a_off = am.entry_arrays(*am.committee_entries(committees))
        t = _batch_arrays(dict(msgs=msgs), n, seed + 5 * s)
        t.update(table=am.table_rows(pks), idx=a_idx.view(np.int32), seg_off=a_off, grp_off=gm.off_array(grp_off), sig=sig)
        sets.append(t)
        want.append((np.array([ok], dtype=np.int32),))
    return sets, want


# the smallest shapes that take two accumulation levels: more than msm::RUN = 32 records (shape[1]); the smaller call takes one
CASES = [
    Case("g1_scaled_segment_sum-seg5-n40", ["zkp_g1_scaled_segment_sum_batch_dev"], "g1_scaled_segment_sum",
         lambda hh, shape, seed: _sum_sets(shape[0], shape[1], seed),
         lambda e, t, sh: e.g1_scaled_segment_sum(t["pts"], t["rand"], t["seg_off"], inf=t["inf"]), (5, 40), (2, 5)),
    Case("bls_verify_grouped-m3-n40", ["zkp_bls_verify_grouped_batch_dev"], "bls_verify_grouped", lambda hh, shape, seed: _verify_sets(shape[0], shape[1], seed),
         lambda e, t, sh: (e.bls_verify_grouped(t["pk"], t["grp_off"], t["msgs"], t["sig"], t["dst"], offsets=t["offsets"], rand=t["rand"]),), (3, 40), (2, 6)),
    Case("bls_fast_aggregate_verify_grouped-m3-idx40", ["zkp_bls_fast_aggregate_verify_grouped_batch_dev"], "bls_fast_aggregate_verify_grouped",
         lambda hh, shape, seed: _aggregate_sets(shape[0], shape[1], seed),
         lambda e, t, sh: (e.bls_fast_aggregate_verify_grouped(t["table"], t["idx"], t["seg_off"], t["grp_off"], t["msgs"], t["sig"], t["dst"],
                                                               offsets=t["offsets"], rand=t["rand"]),), (3, 40), (2, 10)),
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
