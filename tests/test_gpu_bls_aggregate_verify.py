"""AggregateVerify (zkp_bls_aggregate_verify_batch) on one MI355X through the C ABI (run with -m gpu).  Keys, messages and signatures are
made by the MODEL (tests/agg_g2_model.py: individual signatures [sk_i] H(m_i) on Python integers, summed by the model), never by the
library; every case goes through bls_aggregate_verify_batch in the host and the _dev flavour (one pairing product under a random linear
combination; k_aggv_expand builds what the driver reads) and through bls_aggregate_verify_each (one bls_verify call per segment on an
expansion built on the host: a path that never runs k_aggv_expand)."""
import random

import numpy as np
import pytest

import agg_g2_model as a2
import agg_model as am
import bls12_381_model as m
import bls_replay_cases as brc
import h2c_model as h
import outside_groups as og
from test_gpu_bls_aggregate import _dev, _down
from test_gpu_segment_sum import MALFORMED

pytestmark = pytest.mark.gpu
DST = a2.DST
SIZES = {1: [4], 5: [3, 7, 1, 2, 5], 65: [(3 * i) % 7 + 1 for i in range(65)]}       # 65: every size from 1 to 7


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def _batch(n):
    return a2.aggregate_verify_batch(SIZES[n])


def verify_all(eng, pk, msgs, seg_off, sig, want_all, want_each=None, rand=None, host=True, each=True, **kw):
    """seg_off: a list.  The _dev flavour, then (unless the host flavour refuses such input) the host flavour and the per-segment path"""
    import zkvm_pairings_amd as z
    n = len(seg_off) - 1
    a_off = np.array(seg_off, dtype=np.uint64)
    rand = am.rand_rows(n, 77) if rand is None else rand
    buf, off = brc.pack(msgs)
    kd = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    flag = eng.bls_aggregate_verify(_dev(pk), _dev(buf), _dev(a_off), _dev(sig), DST, offsets=_dev(off), rand=_dev(rand), **kd)
    assert bool(flag.cpu().numpy()[0]) is want_all, "_dev flavour"
    if not host:
        return
    assert z.bls_aggregate_verify_batch(pk, msgs, a_off, sig, DST, rand=rand, engine=eng, **kw) is want_all, "host flavour"
    if each:
        got = z.bls_aggregate_verify_each(pk, msgs, a_off, sig, DST, engine=eng, **kw)
        assert got.tolist() == list(np.full(n, want_all) if want_each is None else want_each)


@pytest.mark.parametrize("n", [1, 5, 65])
def test_model_aggregated_signatures_verify_and_the_library_aggregates_to_the_same_bytes(eng, n):
    import zkvm_pairings_amd as z
    b = _batch(n)
    assert n != 65 or sorted(set(SIZES[65])) == list(range(1, 8))
    verify_all(eng, b["pk"], b["msgs"], b["seg_off"], b["sig"], True)
    each = a2.g2_rows(b["each"])[0]
    groups = [list(range(lo, hi)) for lo, hi in zip(b["seg_off"][:-1], b["seg_off"][1:])]
    got, inf = z.bls_aggregate_signatures(each, groups, engine=eng)
    assert got.tobytes() == b["sig"].tobytes() and not inf.any()
    got2, _ = z.bls_aggregate_signatures(each, (np.arange(len(b["msgs"]), dtype=np.uint32), np.array(b["seg_off"], dtype=np.uint64)), engine=eng)
    assert got2.tobytes() == b["sig"].tobytes()
    verify_all(eng, b["pk"], b["msgs"], b["seg_off"], got, True, each=False)
    # the definition: bls_verify on the host-built expansion with the same rand rows
    rand = am.rand_rows(n, 5)
    xs, xi, xr = a2.expand_arrays(b["seg_off"], len(b["msgs"]), b["sig"], None, rand)
    assert z.bls_verify_batch(b["pk"], b["msgs"], xs, DST, rand=xr, inf_sig=xi, engine=eng) is True


FORGERIES = ("message", "keys-swapped", "boundary", "filed-under-neighbour")


@pytest.mark.parametrize("kind", FORGERIES)
def test_one_forgery_at_the_first_a_middle_and_the_last_segment(eng, kind):
    n = 5
    b = _batch(n)
    off = b["seg_off"]
    for j in (0, 2, n - 1):
        pk, msgs, seg_off, sig, down = b["pk"], list(b["msgs"]), list(off), b["sig"], [j]
        lo, hi = off[j], off[j + 1]
        if kind == "message":
            msgs[hi - 1] = b"not what was signed"
        elif kind == "keys-swapped":
            k = next(i for i in range(lo + 1, hi) if b["who"][i] != b["who"][lo]) if hi - lo > 1 else None
            if k is None:                                                  # a segment of one pair: its key changes places with a neighbour's
                k = lo - 1 if lo else hi
                down = sorted({j, j - 1 if lo else j + 1})
            assert b["who"][k] != b["who"][lo]
            pk = pk.copy()
            pk[[lo, k]] = pk[[k, lo]]
        elif kind == "boundary":
            t = j if j else 1                                              # the boundary between segments t - 1 and t moves by one
            seg_off[t] += 1 if off[t + 1] - off[t] > 1 else -1
            down = [t - 1, t]
        else:
            t = j + 1 if j + 1 < n else j - 1
            sig = sig.copy()
            sig[[j, t]] = sig[[t, j]]
            down = [j, t]
        verify_all(eng, pk, msgs, seg_off, sig, False, _down(n, *down))


def test_swapped_signatures_fail_with_distinct_rand_rows_and_pass_with_equal_ones(eng):
    """rand'_i = rand_j: with r_0 = r_3 the product cannot tell which of the two segments a signature stands for; a kernel that took the
    row from the message index would give the two segments different scalars and fail"""
    n = 5
    b = _batch(n)
    sig = b["sig"].copy()
    sig[[0, 3]] = sig[[3, 0]]
    verify_all(eng, b["pk"], b["msgs"], b["seg_off"], sig, False, _down(n, 0, 3), rand=am.rand_rows(n, 11))
    rand = am.rand_rows(n, 11)
    rand[3] = rand[0]
    verify_all(eng, b["pk"], b["msgs"], b["seg_off"], sig, True, each=False, rand=rand)
    verify_all(eng, b["pk"], b["msgs"], b["seg_off"], b["sig"], True, rand=rand)


def test_an_empty_segment_at_each_position_fails(eng):
    n = 5
    b = _batch(n)
    ident = am.u64(h.g2_words(None)[0])
    for j in (0, 2, n):
        seg_off = b["seg_off"][:j + 1] + b["seg_off"][j:]                  # an empty segment in front of segment j (j = n: behind the last)
        sig = np.insert(b["sig"], j, b["sig"][0], axis=0)
        verify_all(eng, b["pk"], b["msgs"], seg_off, sig, False, _down(n + 1, j))
        # ... also with the identity as its signature, which an empty product would accept
        sig[j] = ident
        inf_sig = np.zeros(n + 1, dtype=np.uint8)
        inf_sig[j] = 1
        verify_all(eng, b["pk"], b["msgs"], seg_off, sig, False, _down(n + 1, j), inf_sig=inf_sig)


def test_a_flagged_identity_key_inside_a_segment_fails_its_segment(eng):
    n = 5
    b = _batch(n)
    for i, j in ((0, 0), (b["seg_off"][1] + 3, 1), (len(b["msgs"]) - 1, n - 1)):
        inf_pk = np.zeros(len(b["msgs"]), dtype=np.uint8)
        inf_pk[i] = 1
        verify_all(eng, b["pk"], b["msgs"], b["seg_off"], b["sig"], False, _down(n, j), inf_pk=inf_pk)


def test_a_signature_outside_g2_with_and_without_points_checked(eng):
    """a signature on the curve outside G2 fails the points check; with points_checked the verifier trusts it and the product fails all
    the same (tests/test_gpu_bls.py).  points_checked on sound input changes nothing, and an empty segment is no part of the skipped check"""
    n = 5
    b = _batch(n)
    outside = [q for q in og.g2_points().values() if q is not None and m.g2_on_curve(q) and not m.g2_torsion_free(q)]
    assert outside
    for j in (0, 2, n - 1):
        sig = b["sig"].copy()
        sig[j] = am.u64(h.g2_words(outside[0])[0])
        verify_all(eng, b["pk"], b["msgs"], b["seg_off"], sig, False, _down(n, j))
        verify_all(eng, b["pk"], b["msgs"], b["seg_off"], sig, False, _down(n, j), points_checked=True)
    verify_all(eng, b["pk"], b["msgs"], b["seg_off"], b["sig"], True, points_checked=True)
    seg_off = b["seg_off"] + [b["seg_off"][-1]]
    sig = np.insert(b["sig"], n, b["sig"][0], axis=0)
    verify_all(eng, b["pk"], b["msgs"], seg_off, sig, False, _down(n + 1, n), points_checked=True)


def test_a_zero_row_of_rand_fails_and_the_empty_batch_holds(eng):
    import zkvm_pairings_amd as z
    n = 5
    b = _batch(n)
    for j in (0, 2, n - 1):
        rand = am.rand_rows(n, 31 + j)
        rand[j] = 0
        verify_all(eng, b["pk"], b["msgs"], b["seg_off"], b["sig"], False, np.ones(n, dtype=bool), rand=rand)
    none_pk, none_sig = np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64)
    assert z.bls_aggregate_verify_batch(none_pk, [], [0], none_sig, DST, engine=eng) is True
    assert z.bls_aggregate_verify_each(none_pk, [], [0], none_sig, DST, engine=eng).tolist() == []
    verify_all(eng, none_pk, [], [0], none_sig, True, host=False)
    # signatures and no message: every segment is empty
    verify_all(eng, none_pk, [], [0, 0, 0], b["sig"][:2], False, np.zeros(2, dtype=bool))


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_seg_off_gives_zero_raises_the_validation_word_and_the_host_flavour_refuses(kind):
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import PairingEngine
    from zkvm_pairings_amd._lib import ZkpError
    b = a2.aggregate_verify_batch([3, 7, 1, 2, 5, 8, 8, 8, 3])                 # 45 messages: the offsets of MALFORMED name three segments over 45
    assert len(b["msgs"]) == 45
    sound = [0, 5, 9, 45]
    each = a2.g2_rows(b["each"])[0]
    sig3 = a2.g2_rows([a2.g2_sum(b["each"][lo:hi]) for lo, hi in zip(sound[:-1], sound[1:])])[0]
    off = MALFORMED[kind]
    e = PairingEngine(0, validate=True)
    try:
        verify_all(e, b["pk"], b["msgs"], off, sig3, False, host=False)
        assert e.take_validation_status() is True
        verify_all(e, b["pk"], b["msgs"], sound, sig3, True, host=False)      # the next call is not tainted
        assert e.take_validation_status() is False
        with pytest.raises(ZkpError) as err:
            z.bls_aggregate_verify_batch(b["pk"], b["msgs"], np.array(off, dtype=np.uint64), sig3, DST, engine=e)
        assert err.value.status == -1
        with pytest.raises(ValueError):
            z.bls_aggregate_verify_each(b["pk"], b["msgs"], off, sig3, DST, engine=e)
    finally:
        e.close()
    e = PairingEngine(0)
    try:
        verify_all(e, b["pk"], b["msgs"], off, sig3, False, host=False)       # without validation mode: the same answer, no word
        assert e.take_validation_status() is False
        # messages and no signature: malformed
        flag = e.bls_aggregate_verify(_dev(b["pk"]), _dev(brc.pack(b["msgs"])[0]), _dev(np.zeros(1, dtype=np.uint64)), _dev(np.zeros((0, 24), dtype=np.uint64)),
                                      DST, offsets=_dev(brc.pack(b["msgs"])[1]), rand=_dev(np.zeros((0, 2), dtype=np.uint64)))
        assert int(flag.cpu().numpy()[0]) == 0
    finally:
        e.close()
    assert each.shape == (45, 24)


def test_the_synthetic_instance_verifies_and_a_swap_does_not(eng):
    import zkvm_pairings_amd as z
    sizes = [1, 4, 2]
    sks, pks, msgs, seg_off, sigs = z.synthetic.bls_aggregate_verify_instance(sizes, seed=0x5EED, engine=eng)
    ints = [z.synthetic.scalar_to_int(r) for r in sks]
    assert seg_off.tolist() == [0, 1, 5, 7] and len(set(msgs)) == 7
    want = [a2.g2_sum(am.sign(msgs[i], ints[i]) for i in range(lo, hi)) for lo, hi in zip([0, 1, 5], [1, 5, 7])]
    assert sigs.tobytes() == a2.g2_rows(want)[0].tobytes()
    assert z.bls_aggregate_verify_batch(pks, msgs, seg_off, sigs, DST, engine=eng) is True
    assert z.bls_aggregate_verify_each(pks, msgs, seg_off, sigs, DST, engine=eng).tolist() == [True] * 3
    assert z.bls_aggregate_verify_batch(pks, msgs, seg_off, sigs[[1, 0, 2]], DST, engine=eng) is False


def test_one_message_above_the_slice_of_bls_verify_with_a_segment_across_the_boundary(eng):
    """n_msg = 2^17 + 6 pairs drawn from the model-signed pool of tests/slice_pools.py, segments of 1, 2, 3, 1, 2, 3, ... pairs, the
    aggregate signatures summed by the model once per distinct combination; one segment holds messages 2^17 - 1 and 2^17.  The answer is
    compared with bls_verify on the host-built expansion, sound and with one forged message on each side of the boundary"""
    import slice_pools as sp
    import zkvm_pairings_amd as z
    call = sp.verify_call()
    pool = call.pool["pool"]
    n_msg = sp.VERIFY_N
    assert n_msg == (1 << 17) + 6
    lens = []
    while sum(lens) < n_msg:
        lens.append(min(1 + len(lens) % 3, n_msg - sum(lens)))
    seg_off = np.zeros(len(lens) + 1, dtype=np.uint64)
    seg_off[1:] = np.cumsum(lens)
    n = len(lens)
    cross = int(np.searchsorted(seg_off, 1 << 17, side="right")) - 1
    assert seg_off[cross] < (1 << 17) < seg_off[cross + 1], "no segment straddles message 2^17"
    idx = call.idx
    sums = {}
    sig = np.empty((n, 24), dtype=np.uint64)
    for j in range(n):
        key = tuple(sorted(int(v) for v in idx[int(seg_off[j]):int(seg_off[j + 1])]))
        if key not in sums:
            sums[key] = am.u64(h.g2_words(a2.g2_sum(pool[i][3] for i in key))[0])
        sig[j] = sums[key]
    pk, rand = call.arg("pk"), am.rand_rows(n, 41)
    xs, xi = np.zeros((n_msg, 24), dtype=np.uint64), np.ones(n_msg, dtype=np.uint8)
    xs[:, 12] = 1
    first = seg_off[:-1].astype(np.int64)
    xs[first], xi[first] = sig, 0
    xr = np.repeat(rand, lens, axis=0)
    t_pk, t_off, t_seg, t_sig, t_rand = _dev(pk), _dev(call.offsets), _dev(seg_off), _dev(sig), _dev(rand)
    t_xs, t_xi, t_xr = _dev(xs), _dev(xi), _dev(xr)
    for forged in (None, (1 << 17) - 1, 1 << 17):
        buf = call.msgs if forged is None else sp.forged_messages(call, forged)
        t_buf = _dev(buf)
        got = int(eng.bls_aggregate_verify(t_pk, t_buf, t_seg, t_sig, DST, offsets=t_off, rand=t_rand).cpu().numpy()[0])
        ref = int(eng.bls_verify(t_pk, t_buf, t_xs, DST, offsets=t_off, inf_sig=t_xi, rand=t_xr).cpu().numpy()[0])
        assert got == ref == (1 if forged is None else 0), forged
