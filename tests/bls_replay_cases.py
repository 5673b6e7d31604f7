"""The device-pointer entry points of include/zkp_bls.h (helper of test_gpu_bls_replay.py, test_gpu_h2c.py, test_gpu_bls.py,
test_gpu_call_order_bls.py and test_h2c_cpu.py; not a test module): the Case rows in the form of tests/replay_cases.py and the instances
the BLS tests share.  Expected values never come from the library under test: hashes, points, keys and signatures are made by
tests/h2c_model.py on Python integers."""
import random

import numpy as np

import bls12_381_model as m
import h2c_model as h
import replay_cases as rc
from replay_cases import Case

# every zkp_*_dev( of include/zkp_bls.h has a row below or a written reason here
EXCLUDED = {}

DST = h.ETH_DST


def u64(rows):
    return np.array(rows, dtype=np.uint64)


def pack(msgs, base=0):
    """(buffer uint8 with `base` bytes of filler in front, offsets uint64 (n + 1,))"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[0] = base
    if msgs:
        off[1:] = base + np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    return np.frombuffer(b"\xa5" * base + b"".join(msgs), dtype=np.uint8).copy(), off


def field_rows(msgs, dst):
    return u64([h.f2_words(u0) + h.f2_words(u1) for u0, u1 in (h.hash_to_field_g2(x, dst) for x in msgs)]).reshape(-1, 24)


def point_rows(pts):
    """model points (None: the identity) -> (rows (n, 24), inf (n,))"""
    w = [h.g2_words(p) for p in pts]
    return u64([x for x, _ in w]).reshape(-1, 24), np.array([i for _, i in w], dtype=np.uint8)


def hashed(msg, dst):
    return rc._cached(("h2c", bytes(msg), bytes(dst)), lambda: h.hash_to_g2(msg, dst))


def signed_pool(count=16, seed=0xB15):
    """`count` key pairs with a signed message each, all by the model: [(sk, pk, msg, sig)]"""
    def build():
        rng = random.Random(seed)
        out = []
        for i in range(count):
            sk = rng.randrange(1, h.R_ORDER)
            msg = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 48)))
            out.append((sk, h.sk_to_pk(sk), msg, m.g2_mul(hashed(msg, DST), sk)))
        return out
    return rc._cached(("bls-pool", count, seed), build)


def batch(n, seed=1):
    """n valid signatures drawn from the pool -> dict(pk (n, 12), msgs (list), sig (n, 24), idx)"""
    pool = signed_pool()
    rng = random.Random(seed * 977 + n)
    idx = [rng.randrange(len(pool)) for _ in range(n)]
    if n >= 2 and idx[0] == idx[1]:
        idx[1] = (idx[0] + 1) % len(pool)                       # the first two differ: a swap of neighbours is a forgery
    pk = u64([h.g1_words(pool[i][1])[0] for i in idx]).reshape(-1, 12)
    sig = u64([h.g2_words(pool[i][3])[0] for i in idx]).reshape(-1, 24)
    return dict(pk=pk, msgs=[pool[i][2] for i in idx], sig=sig, idx=idx)


def rand_rows(n, seed):
    rng = random.Random(seed)
    return u64([[rng.randrange(1, 1 << 64), rng.randrange(1, 1 << 64)] for _ in range(n)]).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------------- the replay sets
def _msgs_of(n, seed, total):
    """n messages of `total` bytes together, cut differently for every seed (the buffers of the three sets have one shape)"""
    rng = random.Random(seed)
    cuts = sorted(rng.randrange(total + 1) for _ in range(n - 1))
    data = bytes(rng.randrange(256) for _ in range(total))
    return [data[a:b] for a, b in zip([0] + cuts, cuts + [total])]


def _dst_arr():
    return np.frombuffer(DST, dtype=np.uint8).copy()


def _wide_sets(n, seed):
    rng = random.Random(seed)
    sets, want = [], []
    for _ in range(3):
        vals = [rng.randrange(1 << 512) for _ in range(n)]
        sets.append(dict(data=np.frombuffer(b"".join(v.to_bytes(64, "big") for v in vals), dtype=np.uint8).copy()))
        want.append((u64([h.fp_words(v % h.P) for v in vals]).reshape(-1, 6),))
    return sets, want


def _field_sets(n, seed, points):
    sets, want = [], []
    for s in range(3):
        msgs = _msgs_of(n, seed * 31 + s, 23 * n + 1)
        buf, off = pack(msgs)
        sets.append(dict(msgs=buf, offsets=off, dst=_dst_arr()))
        want.append(point_rows([hashed(x, DST) for x in msgs]) if points else (field_rows(msgs, DST),))
    return sets, want


def _u_of(n, seed):
    g = m.SplitMix64(seed)
    return [((g.below(h.P), g.below(h.P)), (g.below(h.P), g.below(h.P))) for _ in range(n)]


def _map_sets(n, seed):
    sets, want = [], []
    for s in range(3):
        us = _u_of(n, seed * 13 + s)
        if s == 1:
            us[0] = (us[0][0], m.f2_neg(us[0][0]))                  # the identity among the outputs
        sets.append(dict(u=u64([h.f2_words(a) + h.f2_words(b) for a, b in us]).reshape(-1, 24)))
        want.append(point_rows([rc._cached(("map", a, b), lambda a=a, b=b: h.map_from_fields(a, b)) for a, b in us]))
    return sets, want


def _clear_sets(n, seed):
    sets, want = [], []
    for s in range(3):
        pts = [h.iso3(h.sswu(a)[0]) for a, _ in _u_of(n, seed * 17 + s)]
        inf = np.zeros(n, dtype=np.uint8)
        if s == 2:
            pts[-1] = None
        rows, inf = point_rows(pts)
        sets.append(dict(pts=rows, inf=inf))
        want.append(point_rows([rc._cached(("clear", p), lambda p=p: h.clear_cofactor_psi(p)) for p in pts]))
    return sets, want


def _verify_sets(n, seed):
    """A and C hold: B has one message byte changed (messages of one length per position, so that the buffers keep their shape)"""
    sets, want = [], []
    for s in range(3):
        b = batch(n, seed + s)
        msgs = list(b["msgs"])
        ok = 1
        if s == 1:
            j = max(range(n), key=lambda i: len(msgs[i]))
            msgs[j] = bytes([msgs[j][0] ^ 1]) + msgs[j][1:] if msgs[j] else b"\x01"
            ok = 0
        buf, off = pack(msgs)
        pad = np.zeros(48 * n, dtype=np.uint8)
        pad[:buf.size] = buf
        sets.append(dict(pk=b["pk"], msgs=pad, offsets=off, dst=_dst_arr(), sig=b["sig"], rand=rand_rows(n, seed + 5 * s)))
        want.append((np.array([ok], dtype=np.int32),))
    return sets, want


CASES = [
    Case("fp_from_wide_be-n5", ["zkp_fp_from_wide_be_batch_dev"], "fp_from_wide_be", lambda hh, shape, seed: _wide_sets(shape[0], seed),
         lambda e, t, sh: (e.fp_from_wide_be(t["data"]),), (5,), (2,)),
    Case("hash_to_field_g2-n5", ["zkp_hash_to_field_g2_batch_dev"], "hash_to_field_g2", lambda hh, shape, seed: _field_sets(shape[0], seed, False),
         lambda e, t, sh: (e.hash_to_field_g2(t["msgs"], t["dst"], offsets=t["offsets"]),), (5,), (2,)),
    Case("g2_map_from_fields-n3", ["zkp_g2_map_from_fields_batch_dev"], "g2_map_from_fields", lambda hh, shape, seed: _map_sets(shape[0], seed),
         lambda e, t, sh: e.g2_map_from_fields(t["u"]), (3,), (1,)),
    Case("g2_clear_cofactor-n3", ["zkp_g2_clear_cofactor_batch_dev"], "g2_clear_cofactor", lambda hh, shape, seed: _clear_sets(shape[0], seed),
         lambda e, t, sh: e.g2_clear_cofactor(t["pts"], t["inf"]), (3,), (1,)),
    Case("hash_to_g2-n3", ["zkp_hash_to_g2_batch_dev"], "hash_to_g2", lambda hh, shape, seed: _field_sets(shape[0], seed, True),
         lambda e, t, sh: e.hash_to_g2(t["msgs"], t["dst"], offsets=t["offsets"]), (3,), (1,)),
    Case("bls_verify-n6", ["zkp_bls_verify_batch_dev"], "bls_verify", lambda hh, shape, seed: _verify_sets(shape[0], seed),
         lambda e, t, sh: (e.bls_verify(t["pk"], t["msgs"], t["sig"], t["dst"], offsets=t["offsets"], rand=t["rand"]),), (6,), (2,)),
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
