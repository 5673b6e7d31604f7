"""The model of include/zkp_bls_agg.h on Python integers (helper of the test_*agg* and test_gpu_segment_sum / test_gpu_bls_aggregate
modules; not a test module): segment sums of signed table rows with tests/golden/bls12_381_model.py, committee_entries as the header
states it, the index kernels' keys and values, and the key table with model-signed aggregates the GPU tests share.  Nothing here calls
the library under test."""
import random

import numpy as np

import bls12_381_model as m
import h2c_model as h
import replay_cases as rc

SIGN = 0x80000000
ROW = 0x7FFFFFFF
KEY_NONE = 0x7FFFFFFF
DST = h.ETH_DST


def u64(rows):
    return np.array(rows, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------------- entries
def committee_entries(committees, bits=None, absent_from=None):
    """(idx as a list of ints, seg_off as a list): the members whose bit is set, or the total row minus the listed absentees"""
    assert bits is None or absent_from is None
    out = []
    for i, c in enumerate(committees):
        c = [int(r) for r in c]
        if bits is not None:
            assert len(bits[i]) == len(c)
            c = [r for r, b in zip(c, bits[i]) if b]
        if absent_from is not None:
            total = absent_from if isinstance(absent_from, int) else absent_from[i]
            c = [int(total)] + [r | SIGN for r in c]
        out.append(c)
    seg_off = [0]
    for c in out:
        seg_off.append(seg_off[-1] + len(c))
    return [r for c in out for r in c], seg_off


def offsets_sound(seg_off, n_idx):
    return seg_off[0] == 0 and seg_off[-1] == n_idx and all(a <= b for a, b in zip(seg_off, seg_off[1:]))


def keys_values(idx, seg_off, n_table):
    """what k_agg_check and k_agg_keys leave: (keys, vals, status, word)"""
    n_seg = len(seg_off) - 1
    if not offsets_sound(seg_off, len(idx)):
        return [KEY_NONE] * len(idx), [0] * len(idx), [0] * n_seg, 1
    keys, vals, status = [], [], [0] * n_seg
    for j in range(n_seg):
        for e in range(seg_off[j], seg_off[j + 1]):
            row = idx[e] & ROW
            if row >= n_table:
                status[j], row = 1, 0
            keys.append(j)
            vals.append(row | (idx[e] & SIGN))
    return keys, vals, status, 0


# ------------------------------------------------------------------------------------------------------------------- sums
def segment_sums(table, idx, seg_off):
    """table: model points -> (points (None: the identity), status): the behaviour of the _dev flavour on any input"""
    n_seg = len(seg_off) - 1
    if not offsets_sound(seg_off, len(idx)):
        return [None] * n_seg, [1] * n_seg
    pts, status = [], []
    for j in range(n_seg):
        acc, bad = None, 0
        for e in idx[seg_off[j]:seg_off[j + 1]]:
            row = e & ROW
            if row >= len(table):
                bad = 1
                continue
            q = table[row]
            acc = m.g1_add(acc, m.g1_neg(q) if e & SIGN else q)
        pts.append(None if bad else acc)
        status.append(bad)
    return pts, status


def g1_rows(pts):
    """model points (None: the identity) -> (rows (n, 12), inf (n,))"""
    w = [h.g1_words(p) for p in pts]
    return u64([x for x, _ in w]).reshape(-1, 12), np.array([i for _, i in w], dtype=np.uint8)


def sum_rows(table, idx, seg_off):
    """(out (n_seg, 12), out_inf, status) as the library writes them"""
    pts, status = segment_sums(table, idx, seg_off)
    rows, inf = g1_rows(pts)
    return rows, inf, np.array(status, dtype=np.uint8)


def entry_arrays(idx, seg_off):
    return np.array(idx, dtype=np.uint32), np.array(seg_off, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------------- the shared table
def _doublings(key, base, add):
    """base, 2 base, 4 base, ...: 255 of them, so that a multiple costs one addition per set bit of the scalar"""
    def build():
        out = [base]
        for _ in range(254):
            out.append(add(out[-1], out[-1]))
        return out
    return rc._cached(("agg-doublings", key), build)


def _multiple(powers, k, add):
    acc = None
    for i, p in enumerate(powers):
        if (k >> i) & 1:
            acc = add(acc, p)
    return acc


def public_key(sk):
    """[sk] g1, through the doublings of the generator"""
    return _multiple(_doublings("g1", m.G1_GEN, m.g1_add), sk % h.R_ORDER, m.g1_add)


def key_table(count, seed=0xA66):
    """`count` key pairs by the model: (sks, pks); pk_i = [sk_i] g1, the secret keys from the seed, the table the same for every count"""
    def build():
        rng = random.Random(seed)
        sks = [rng.randrange(1, h.R_ORDER) for _ in range(count)]
        return sks, [public_key(sk) for sk in sks]
    return rc._cached(("agg-table", count, seed), build)


def table_rows(pks):
    return g1_rows(pks)[0]


def hashed(msg):
    return rc._cached(("h2c", bytes(msg), bytes(DST)), lambda: h.hash_to_g2(msg, DST))


MESSAGES = [b"", b"attestation", bytes(range(32)), b"sync committee, slot 7", b"\x00" * 55, bytes(range(64, 0, -1)), b"m", b"another block root"]


def sign(msg, sk):
    """[sk] H(msg) by the model, through the doublings of H(msg) (the batches sign the few MESSAGES many times)"""
    return _multiple(_doublings(("h", bytes(msg)), hashed(msg), m.g2_add), sk % h.R_ORDER, m.g2_add)


def aggregate_batch(n, n_table=64, seed=1, sizes=None):
    """n model-signed aggregates over key_table(n_table): committee i has sizes[i] members (by default 1 .. 40 from the seed, all
    different; committees 0 and 1 have at least two), a message of MESSAGES (neighbours differ) and the signature [sum of its secret
    keys] H(m) -> dict(committees, msgs, sig (n, 24))"""
    def build():
        sks, _ = key_table(n_table)
        rng = random.Random(seed * 7919 + n)
        committees, msgs, sigs = [], [], []
        for i in range(n):
            k = sizes[i] if sizes else rng.randrange(2 if i < 2 else 1, 41)
            c = rng.sample(range(n_table), k)
            msg = MESSAGES[(i + seed) % len(MESSAGES)]
            committees.append(c)
            msgs.append(msg)
            sigs.append(sign(msg, sum(sks[r] for r in c)))
        return dict(committees=committees, msgs=msgs, sig=u64([h.g2_words(s)[0] for s in sigs]).reshape(-1, 24))
    return rc._cached(("agg-batch", n, n_table, seed, tuple(sizes) if sizes else None), build)


def rand_rows(n, seed):
    rng = random.Random(seed)
    return u64([[rng.randrange(1, 1 << 64), rng.randrange(1, 1 << 64)] for _ in range(n)]).reshape(-1, 2)
