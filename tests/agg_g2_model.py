"""The model of include/zkp_bls_agg_g2.h on Python integers (helper of the test_*agg_g2* and test_gpu_g2_segment_sum /
test_gpu_bls_minsig_aggregate / test_gpu_bls_aggregate_verify modules; not a test module): G2 segment sums of signed table rows with
tests/golden/bls12_381_model.py and the status rules of tests/agg_model.py, the expansion of AggregateVerify as lists, a min-sig key
table (pk = [sk] g2) with aggregates signed through tests/h2g1_model.py, and AggregateVerify instances whose signatures are sums of
individual model signatures.  Nothing here calls the library under test."""
import random

import numpy as np

import agg_model as am
import bls12_381_model as m
import h2c_model as h
import h2g1_model as g1h
import replay_cases as rc

SIGN, ROW = am.SIGN, am.ROW
DST = h.ETH_DST                                      # the min-pk layout: signatures in G2
MINSIG_DST = g1h.QUICKNET_DST                        # the min-sig layout: signatures in G1
u64 = am.u64


# ------------------------------------------------------------------------------------------------------------------- G2 sums
def g2_sum(points):
    acc = None
    for p in points:
        acc = m.g2_add(acc, p)
    return acc


def segment_sums(table, idx, seg_off):
    """table: model points of the twist -> (points (None: the identity), status): agg_model.segment_sums with the law of G2"""
    n_seg = len(seg_off) - 1
    if not am.offsets_sound(seg_off, len(idx)):
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
            acc = m.g2_add(acc, m.g2_neg(q) if e & SIGN else q)
        pts.append(None if bad else acc)
        status.append(bad)
    return pts, status


def g2_rows(pts):
    """model points (None: the identity) -> (rows (n, 24), inf (n,))"""
    w = [h.g2_words(p) for p in pts]
    return u64([x for x, _ in w]).reshape(-1, 24), np.array([i for _, i in w], dtype=np.uint8)


def sum_rows(table, idx, seg_off):
    """(out (n_seg, 24), out_inf, status) as the library writes them"""
    pts, status = segment_sums(table, idx, seg_off)
    rows, inf = g2_rows(pts)
    return rows, inf, np.array(status, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------- the expansion
def expansion(seg_off, n_msg, n):
    """what k_aggv_expand leaves, as lists per message: (segment whose rand row the message gets, segment whose signature it gets or
    None for the flagged identity, the call's word).  A malformed call: rand row None (the kernel writes (1, 0)), no signature"""
    if len(seg_off) != n + 1 or not am.offsets_sound(seg_off, n_msg):
        return [None] * n_msg, [None] * n_msg, 1
    seg, first = [None] * n_msg, [None] * n_msg
    for j in range(n):
        for i in range(seg_off[j], seg_off[j + 1]):
            seg[i] = j
            first[i] = j if i == seg_off[j] else None
    return seg, first, 0


def expand_arrays(seg_off, n_msg, sig, inf_sig, rand):
    """the three arrays zkp_bls_verify_batch's driver reads: (sig' (n_msg, 24), inf_sig' (n_msg,), rand' (n_msg, 2)); sig (n, 24),
    inf_sig (n,) or None, rand (n, 2)"""
    n = len(seg_off) - 1
    seg, first, _ = expansion(list(seg_off), n_msg, n)
    xs = np.zeros((n_msg, 24), dtype=np.uint64)
    xs[:, 12] = 1
    xi = np.ones(n_msg, dtype=np.uint8)
    xr = np.zeros((n_msg, 2), dtype=np.uint64)
    xr[:, 0] = 1
    for i in range(n_msg):
        if seg[i] is not None:
            xr[i] = rand[seg[i]]
        if first[i] is not None:
            xs[i] = sig[first[i]]
            xi[i] = 0 if inf_sig is None else inf_sig[first[i]]
    return xs, xi, xr


# ------------------------------------------------------------------------------------------------------------------- plain BLS on the model
def bls_verify_model(pks, msgs, sigs):
    """prod_i e(pk_i, H(m_i)) == e(g1, sum_i sig_i): the batch equation of zkp_bls_verify_batch with every r_i = 1 (model points;
    None: the identity, which as a key fails)"""
    if any(p is None for p in pks):
        return False
    lhs = m.f12_one()
    for pk, msg in zip(pks, msgs):
        lhs = m.f12_mul(lhs, m.pairing(pk, am.hashed(msg)))
    total = g2_sum(sigs)
    rhs = m.f12_one() if total is None else m.pairing(m.G1_GEN, total)
    return lhs == rhs


def aggregate_verify_model(pks, msgs, seg_off, sigs):
    """the per-segment definition: signature j against the product over its pairs; an empty segment fails"""
    out = []
    for j in range(len(seg_off) - 1):
        lo, hi = seg_off[j], seg_off[j + 1]
        out.append(hi > lo and bls_verify_model(pks[lo:hi], msgs[lo:hi], [sigs[j]]))
    return out


# ------------------------------------------------------------------------------------------------------------------- the min-sig table
def minsig_public_key(sk):
    """[sk] g2, through the doublings of the generator"""
    return am._multiple(am._doublings("g2", m.G2_GEN, m.g2_add), sk % h.R_ORDER, m.g2_add)


def minsig_key_table(count, seed=0xA67):
    """`count` key pairs by the model: (sks, pks); pk_i = [sk_i] g2"""
    def build():
        rng = random.Random(seed)
        sks = [rng.randrange(1, h.R_ORDER) for _ in range(count)]
        return sks, [minsig_public_key(sk) for sk in sks]
    return rc._cached(("agg2-table", count, seed), build)


def g2_table(count):
    """the G2 points the segment-sum tests gather: the min-sig keys (any points of G2 do)"""
    return minsig_key_table(count)[1]


def minsig_hashed(msg, dst=MINSIG_DST):
    return rc._cached(("h2g1", bytes(msg), bytes(dst)), lambda: g1h.hash_to_g1(msg, dst))


def minsig_sign(msg, sk, dst=MINSIG_DST):
    """[sk] H(msg) in G1 by the model, through the doublings of H(msg)"""
    return am._multiple(am._doublings(("h1", bytes(msg), bytes(dst)), minsig_hashed(msg, dst), g1h.e_add), sk % h.R_ORDER, g1h.e_add)


def minsig_aggregate_batch(n, n_table=64, seed=1, sizes=None):
    """agg_model.aggregate_batch for G2 keys -> dict(committees, msgs, sig (n, 12))"""
    def build():
        sks, _ = minsig_key_table(n_table)
        rng = random.Random(seed * 7919 + n)
        committees, msgs, sigs = [], [], []
        for i in range(n):
            k = sizes[i] if sizes else rng.randrange(2 if i < 2 else 1, 41)
            c = rng.sample(range(n_table), k)
            msg = am.MESSAGES[(i + seed) % len(am.MESSAGES)]
            committees.append(c)
            msgs.append(msg)
            sigs.append(minsig_sign(msg, sum(sks[r] for r in c)))
        return dict(committees=committees, msgs=msgs, sig=u64([h.g1_words(s)[0] for s in sigs]).reshape(-1, 12))
    return rc._cached(("agg2-batch", n, n_table, seed, tuple(sizes) if sizes else None), build)


# ------------------------------------------------------------------------------------------------------------------- AggregateVerify
def signed(msg, r, n_keys):
    """[sk_r] H(msg) by key r of agg_model.key_table(n_keys): the batches sign the few (message, key) pairs many times"""
    return rc._cached(("aggv-sign", bytes(msg), r, n_keys), lambda: am.sign(msg, am.key_table(n_keys)[0][r]))


def aggregate_verify_batch(sizes, n_keys=8, seed=1):
    """one aggregate signature per entry of sizes over sizes[j] pairs: the keys are drawn from agg_model.key_table(n_keys), the messages
    from agg_model.MESSAGES so that the messages of one segment differ (sizes up to 8), each pair is signed by the model, [sk_i] H(m_i),
    and the model sums the signatures.  -> dict(sks, pk (n_msg, 12), pts (key points), msgs, seg_off (list), each (model signatures per
    message), sig_pts (n model points), sig (n, 24))"""
    def build():
        sks, pks = am.key_table(n_keys)
        rng = random.Random(seed * 104729 + len(sizes))
        who, msgs, seg_off = [], [], [0]
        for k in sizes:
            assert k <= len(am.MESSAGES)
            who += [rng.randrange(n_keys) for _ in range(k)]
            msgs += rng.sample(am.MESSAGES, k)
            seg_off.append(seg_off[-1] + k)
        each = [signed(x, r, n_keys) for x, r in zip(msgs, who)]
        sig_pts = [g2_sum(each[a:b]) for a, b in zip(seg_off[:-1], seg_off[1:])]
        return dict(sks=[sks[r] for r in who], who=who, pts=[pks[r] for r in who], pk=am.g1_rows([pks[r] for r in who])[0].copy(), msgs=msgs,
                    seg_off=seg_off, each=each, sig_pts=sig_pts, sig=g2_rows(sig_pts)[0])
    return rc._cached(("aggv-batch", tuple(sizes), n_keys, seed), build)
