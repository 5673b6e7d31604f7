"""The model of include/zkp_bls_grouped.h on Python integers (helper of the test_*grp* / test_gpu_scaled_segment_sum / test_gpu_bls_grouped
modules; not a test module): the scalar a + b z^2, scaled segment sums, group_by_message as the header states it, the index kernels' keys,
the two pairing products of the verifier, and model-signed batches ordered by message.  Points of the sums are given by their discrete
logarithms (the keys of tests/agg_model.py's table), so a sum of scaled points is ONE multiple of the generator: sum [r_i] [s_i] g1 =
[sum r_i s_i] g1.  Nothing here calls the library under test."""
import random

import numpy as np

import agg_model as am
import bls12_381_model as m
import h2c_model as h
import replay_cases as rc

KEY_NONE = 0x7FFFFFFF
KEY_FLAG = 0x80000000
Z2 = m.BLS_X * m.BLS_X
DST = h.ETH_DST
R = h.R_ORDER


def scalar(a, b):
    """r = a + b z^2: below the group order for 64-bit a and b"""
    r = a + b * Z2
    assert r < R
    return r


def offsets_sound(seg_off, n):
    return seg_off[0] == 0 and seg_off[-1] == n and all(a <= b for a, b in zip(seg_off, seg_off[1:]))


def keys(n, seg_off):
    """what k_grp_check and k_grp_keys leave: (keys, word)"""
    if not offsets_sound(seg_off, n):
        return [KEY_NONE] * n, 1
    out = []
    for g in range(len(seg_off) - 1):
        out += [g | KEY_FLAG] * (seg_off[g + 1] - seg_off[g])
    return out, 0


def group_by_message(messages):
    """(perm, distinct, grp_off): distinct messages in the order of their first appearance, members in their order"""
    distinct = []
    for x in messages:
        if bytes(x) not in distinct:
            distinct.append(bytes(x))
    members = [[i for i, x in enumerate(messages) if bytes(x) == d] for d in distinct]
    grp_off = [0]
    for x in members:
        grp_off.append(grp_off[-1] + len(x))
    return [i for x in members for i in x], distinct, grp_off


# ------------------------------------------------------------------------------------------------------------------- sums
def scaled_segment_sums(logs, rand, seg_off):
    """logs[i]: the discrete logarithm of point i (None: the identity); rand[i] = (a, b) -> (points (None: the identity), status): the
    behaviour of the _dev flavour on any input"""
    n_seg = len(seg_off) - 1
    if not offsets_sound(seg_off, len(logs)):
        return [None] * n_seg, [1] * n_seg
    pts = []
    for g in range(n_seg):
        k = sum(scalar(*rand[i]) * logs[i] for i in range(seg_off[g], seg_off[g + 1]) if logs[i] is not None) % R
        pts.append(am.public_key(k) if k else None)
    return pts, [0] * n_seg


def sum_rows(logs, rand, seg_off):
    """(out (n_seg, 12), out_inf, status) as the library writes them"""
    pts, status = scaled_segment_sums(logs, rand, seg_off)
    rows, inf = am.g1_rows(pts)
    return rows, inf, np.array(status, dtype=np.uint8)


def point_rows(logs):
    """(rows (n, 12), inf (n,)) of the points [log] g1; an identity input is written (0, 1) with its byte set"""
    return am.g1_rows([None if k is None else am.public_key(k) for k in logs])


def rand_rows(n, seed):
    return am.rand_rows(n, seed)


def rand_pairs(rand):
    return [(int(a), int(b)) for a, b in np.asarray(rand, dtype=np.uint64).reshape(-1, 2)]


# ------------------------------------------------------------------------------------------------------------------- the two products
def product_ungrouped(pks, msgs, sigs, rand):
    """prod_i e([r_i] pk_i, H(m_i)) e(-g1, sum_i [r_i] sig_i) before the final exponentiation, one message per signature"""
    pairs, s = [], None
    for pk, msg, sig, ab in zip(pks, msgs, sigs, rand):
        r = scalar(*ab)
        pairs.append((m.g1_mul(pk, r), am.hashed(msg)))
        s = m.g2_add(s, m.g2_mul(sig, r))
    pairs.append((m.g1_neg(m.G1_GEN), s))
    return m.multi_miller_loop([p for p in pairs if p[0] is not None and p[1] is not None])


def product_grouped(pks, distinct, grp_off, sigs, rand):
    """prod_g e(sum_{i in g} [r_i] pk_i, H(m_g)) e(-g1, sum_i [r_i] sig_i): m + 1 pairs"""
    pairs, s = [], None
    for g, msg in enumerate(distinct):
        a = None
        for i in range(grp_off[g], grp_off[g + 1]):
            a = m.g1_add(a, m.g1_mul(pks[i], scalar(*rand[i])))
        pairs.append((a, am.hashed(msg)))
    for sig, ab in zip(sigs, rand):
        s = m.g2_add(s, m.g2_mul(sig, scalar(*ab)))
    pairs.append((m.g1_neg(m.G1_GEN), s))
    return m.multi_miller_loop([p for p in pairs if p[0] is not None and p[1] is not None])


def is_one(f):
    return m.final_exponentiation(f) == m.f12_one()


# ------------------------------------------------------------------------------------------------------------------- model-signed batches
N_TABLE = 64


def grouped_batch(sizes, seed=1):
    """sum(sizes) model-signed signatures ORDERED BY MESSAGE: group g holds sizes[g] signatures of MESSAGES[g] by keys of
    am.key_table(64) (drawn with repetition across groups, without inside one) -> dict(rows: the signers' table rows, sks, pk (n, 12),
    msgs (the m distinct messages), grp_off, sig (n, 24), expanded: the message of every signature)"""
    def build():
        sks, pks = am.key_table(N_TABLE)
        rng = random.Random(seed * 6151 + sum(sizes))
        rows, expanded, sigs = [], [], []
        for g, k in enumerate(sizes):
            for r in rng.sample(range(N_TABLE), k):
                rows.append(r)
                expanded.append(am.MESSAGES[g])
                sigs.append(am.sign(am.MESSAGES[g], sks[r]))
        grp_off = [0]
        for k in sizes:
            grp_off.append(grp_off[-1] + k)
        return dict(rows=rows, sks=[sks[r] for r in rows], pk=am.table_rows([pks[r] for r in rows]), msgs=list(am.MESSAGES[:len(sizes)]), grp_off=grp_off,
                    sig=am.u64([h.g2_words(s)[0] for s in sigs]).reshape(-1, 24), expanded=expanded)
    return rc._cached(("grp-batch", tuple(sizes), seed), build)


def off_array(off):
    return np.array(off, dtype=np.uint64)
