"""The device-pointer entry points of include/zkp_bls_minsig.h (helper of test_gpu_minsig_replay.py and test_h2g1_cpu.py; not a test
module): the Case rows in the form of tests/replay_cases.py and the instances the replay and call-order tests share.  Expected values
never come from the library under test: hashes, points, keys and signatures are made by tests/h2g1_model.py on Python integers."""
import random

import numpy as np

import bls12_381_model as m
import h2c_model as h
import h2g1_model as g
import replay_cases as rc
from replay_cases import Case

# every zkp_*_dev( of include/zkp_bls_minsig.h has a row below or a written reason here
EXCLUDED = {}

DST = g.QUICKNET_DST


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
    return u64([g.fp_words(u0) + g.fp_words(u1) for u0, u1 in (g.hash_to_field_g1(x, dst) for x in msgs)]).reshape(-1, 12)


def point_rows(pts):
    """model points of E (None: the identity) -> (rows (n, 12), inf (n,))"""
    w = [g.g1_words(p) for p in pts]
    return u64([x for x, _ in w]).reshape(-1, 12), np.array([i for _, i in w], dtype=np.uint8)


def hashed(msg, dst):
    return rc._cached(("h2g1", bytes(msg), bytes(dst)), lambda: g.hash_to_g1(msg, dst))


def signed_pool(count=12, seed=0xB16):
    """`count` key pairs with a signed message each, all by the model: [(sk, pk in G2, msg, sig in G1)]"""
    def build():
        rng = random.Random(seed)
        out = []
        for _ in range(count):
            sk = rng.randrange(1, g.R_ORDER)
            msg = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 48)))
            out.append((sk, g.sk_to_pk(sk), msg, g.e_mul(hashed(msg, DST), sk)))
        return out
    return rc._cached(("minsig-pool", count, seed), build)


def batch(n, seed=1):
    """n valid signatures drawn from the pool -> dict(pk (n, 24), msgs (list), sig (n, 12), idx)"""
    pool = signed_pool()
    rng = random.Random(seed * 977 + n)
    idx = [rng.randrange(len(pool)) for _ in range(n)]
    if n >= 2 and idx[0] == idx[1]:
        idx[1] = (idx[0] + 1) % len(pool)                       # the first two differ: a swap of neighbours is a forgery
    pk = u64([h.g2_words(pool[i][1])[0] for i in idx]).reshape(-1, 24)
    sig = u64([g.g1_words(pool[i][3])[0] for i in idx]).reshape(-1, 12)
    return dict(pk=pk, msgs=[pool[i][2] for i in idx], sig=sig, idx=idx)


def same_key_batch(n, seed=1):
    """n messages of the pool signed by ONE key (the pool's first) -> dict(pk1 (1, 24), pk (n, 24), msgs, sig (n, 12))"""
    pool = signed_pool()
    sk, pk = pool[0][0], pool[0][1]
    rng = random.Random(seed * 733 + n)
    msgs = [pool[rng.randrange(len(pool))][2] for _ in range(n)]
    sigs = [rc._cached(("minsig-same", x), lambda x=x: g.e_mul(hashed(x, DST), sk)) for x in msgs]
    row = u64(h.g2_words(pk)[0]).reshape(1, 24)
    return dict(pk1=row, pk=np.tile(row, (n, 1)), msgs=msgs, sig=u64([g.g1_words(s)[0] for s in sigs]).reshape(-1, 12))


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


def _field_sets(n, seed, points):
    sets, want = [], []
    for s in range(3):
        msgs = _msgs_of(n, seed * 31 + s, 23 * n + 1)
        buf, off = pack(msgs)
        sets.append(dict(msgs=buf, offsets=off, dst=_dst_arr()))
        want.append(point_rows([hashed(x, DST) for x in msgs]) if points else (field_rows(msgs, DST),))
    return sets, want


def _u_of(n, seed):
    rng = random.Random(seed)
    return [(rng.randrange(g.P), rng.randrange(g.P)) for _ in range(n)]


def _map_sets(n, seed):
    sets, want = [], []
    for s in range(3):
        us = _u_of(n, seed * 13 + s)
        if s == 1:
            us[0] = (us[0][0], g.P - us[0][0])                      # the identity among the outputs
        sets.append(dict(u=u64([g.fp_words(a) + g.fp_words(b) for a, b in us]).reshape(-1, 12)))
        want.append(point_rows([rc._cached(("map1", a, b), lambda a=a, b=b: g.map_from_fields(a, b)) for a, b in us]))
    return sets, want


def _clear_sets(n, seed):
    sets, want = [], []
    for s in range(3):
        pts = [g.iso11(g.sswu(a)[0]) for a, _ in _u_of(n, seed * 17 + s)]
        if s == 2:
            pts[-1] = None
        rows, inf = point_rows(pts)
        sets.append(dict(pts=rows, inf=inf))
        want.append(point_rows([rc._cached(("clear1", p), lambda p=p: g.clear_cofactor(p)) for p in pts]))
    return sets, want


def _verify_sets(n, seed, same_key):
    """A and C hold: B has one message byte changed (the buffers keep their shape: the messages are padded to 48 n bytes)"""
    sets, want = [], []
    for s in range(3):
        b = same_key_batch(n, seed + s) if same_key else batch(n, seed + s)
        msgs = list(b["msgs"])
        ok = 1
        if s == 1:
            j = max(range(n), key=lambda i: len(msgs[i]))
            msgs[j] = bytes([msgs[j][0] ^ 1]) + msgs[j][1:] if msgs[j] else b"\x01"
            ok = 0
        buf, off = pack(msgs)
        pad = np.zeros(48 * n, dtype=np.uint8)
        pad[:buf.size] = buf
        sets.append(dict(pk=b["pk1"] if same_key else b["pk"], msgs=pad, offsets=off, dst=_dst_arr(), sig=b["sig"], rand=rand_rows(n, seed + 5 * s)))
        want.append((np.array([ok], dtype=np.int32),))
    return sets, want


CASES = [
    Case("hash_to_field_g1-n5", ["zkp_hash_to_field_g1_batch_dev"], "hash_to_field_g1", lambda hh, shape, seed: _field_sets(shape[0], seed, False),
         lambda e, t, sh: (e.hash_to_field_g1(t["msgs"], t["dst"], offsets=t["offsets"]),), (5,), (2,)),
    Case("g1_map_from_fields-n3", ["zkp_g1_map_from_fields_batch_dev"], "g1_map_from_fields", lambda hh, shape, seed: _map_sets(shape[0], seed),
         lambda e, t, sh: e.g1_map_from_fields(t["u"]), (3,), (1,)),
    Case("g1_clear_cofactor-n3", ["zkp_g1_clear_cofactor_batch_dev"], "g1_clear_cofactor", lambda hh, shape, seed: _clear_sets(shape[0], seed),
         lambda e, t, sh: e.g1_clear_cofactor(t["pts"], t["inf"]), (3,), (1,)),
    Case("hash_to_g1-n3", ["zkp_hash_to_g1_batch_dev"], "hash_to_g1", lambda hh, shape, seed: _field_sets(shape[0], seed, True),
         lambda e, t, sh: e.hash_to_g1(t["msgs"], t["dst"], offsets=t["offsets"]), (3,), (1,)),
    Case("bls_minsig_verify-n6", ["zkp_bls_minsig_verify_batch_dev"], "bls_minsig_verify", lambda hh, shape, seed: _verify_sets(shape[0], seed, False),
         lambda e, t, sh: (e.bls_minsig_verify(t["pk"], t["msgs"], t["sig"], t["dst"], offsets=t["offsets"], rand=t["rand"]),), (6,), (2,)),
    Case("bls_minsig_verify_samekey-n6", ["zkp_bls_minsig_verify_samekey_batch_dev"], "bls_minsig_verify_samekey",
         lambda hh, shape, seed: _verify_sets(shape[0], seed, True),
         lambda e, t, sh: (e.bls_minsig_verify_samekey(t["pk"], t["msgs"], t["sig"], t["dst"], offsets=t["offsets"], rand=t["rand"]),), (6,), (2,)),
]


def table_c_names():
    return set(n for c in CASES for n in c.c_names)
