"""A batch larger than one slice of the hash-to-G1 pipeline (2^17 messages) assembled from a pool of at most 64 distinct messages by a
pseudo-random index sequence, in the manner of tests/slice_pools.py: the model hashes the pool, not the batch.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

SLICE = 1 << 17
N_SLICED = SLICE + 61
POOL = 64
FIRST_OFFSET = 7                     # the first offset is not zero: the buffer opens with bytes no message owns


def pool_messages():
    """POOL distinct messages of lengths 0 .. 63, every byte from the index"""
    return [bytes((7 * i + 3 * j + 1) & 0xFF for j in range(i)) for i in range(POOL)]


def index_sequence(n=N_SLICED, seed=0x9E3779B97F4A7C15):
    """n indices below POOL from a 64-bit linear congruential generator; both sides of the slice boundary get different ones"""
    out = np.empty(n, dtype=np.int64)
    x = seed
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[i] = x >> 58
    return out


def packed(idx):
    """(buffer uint8, offsets uint64 (n + 1,)) of the messages pool[idx[i]], the first offset FIRST_OFFSET"""
    pool = pool_messages()
    lens = np.array([len(x) for x in pool], dtype=np.uint64)[idx]
    offsets = np.empty(idx.size + 1, dtype=np.uint64)
    offsets[0] = FIRST_OFFSET
    offsets[1:] = FIRST_OFFSET + np.cumsum(lens, dtype=np.uint64)
    buf = np.frombuffer(b"\xEE" * FIRST_OFFSET + b"".join(pool[i] for i in idx), dtype=np.uint8)
    return buf, offsets
