"""zkp_bls_verify_grouped_batch and zkp_bls_fast_aggregate_verify_grouped_batch on one MI355X through the C ABI (run with -m gpu).  Keys and
signatures are made by the MODEL (tests/grp_model.py, tests/agg_model.py), never by the library.  Every case states its expected answer,
asks the grouped call in the _dev and the host flavour, and asks zkp_bls_verify_batch (zkp_bls_fast_aggregate_verify_batch) on the same
signatures with the messages expanded and the same rand: the three must agree."""
import numpy as np
import pytest

import agg_model as am
import bls12_381_model as m
import grp_model as gm
import h2c_model as h
import outside_groups as og
from bls_replay_cases import pack

pytestmark = pytest.mark.gpu
DST = h.ETH_DST
SIZES = [1, 33, 0, 32, 4]          # n = 70, m = 5: a run border inside group 1 and at the start of group 3, a message nobody signed
N = 70


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch():
    return gm.grouped_batch(SIZES)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _expand(msgs, grp_off):
    return [msgs[g] for g in range(len(msgs)) for _ in range(grp_off[g + 1] - grp_off[g])]


def verify(eng, want, pk, grp_off, msgs, sig, rand=None, host=True, ungrouped=True, **kw):
    """want: the stated answer.  The _dev flavour, the host flavour, and bls_verify on the expanded messages"""
    n = pk.shape[0]
    rand = gm.rand_rows(n, 77) if rand is None else rand
    buf, off = pack(msgs)
    kd = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    flag = eng.bls_verify_grouped(_dev(pk), _dev(gm.off_array(grp_off)), _dev(buf), _dev(sig), DST, offsets=_dev(off), rand=_dev(rand), **kd)
    assert bool(flag.cpu().numpy()[0]) is want, "_dev flavour"
    if host:
        assert eng.bls_verify_grouped(pk, gm.off_array(grp_off), msgs, sig, DST, rand=rand, **kw) is want, "host flavour"
    if ungrouped:
        assert eng.bls_verify(pk, _expand(msgs, grp_off), sig, DST, rand=rand, **kw) is want, "bls_verify on the expanded messages"


def test_the_honest_batch_holds(eng, batch):
    import zkvm_pairings_amd as z
    verify(eng, True, batch["pk"], batch["grp_off"], batch["msgs"], batch["sig"])
    # the module function takes the messages per signature, in any order, and sorts
    order = np.random.RandomState(70).permutation(N)
    msgs = [batch["expanded"][i] for i in order]
    assert z.bls_verify_grouped_batch(batch["pk"][order], msgs, batch["sig"][order], DST, rand=gm.rand_rows(N, 5), engine=eng) is True
    perm, distinct, grp_off = z.group_by_message(msgs)
    assert (perm.tolist(), distinct, grp_off.tolist()) == gm.group_by_message(msgs)


@pytest.mark.parametrize("where", [0, N - 1])
def test_one_forged_signature_in_the_first_and_in_the_last_group_fails(eng, batch, where):
    sig = batch["sig"].copy()
    sig[where] = am.u64(h.g2_words(am.sign(batch["expanded"][where], batch["sks"][where] + 1))[0])
    verify(eng, False, batch["pk"], batch["grp_off"], batch["msgs"], sig)


def test_two_signatures_of_one_group_swapped_fail(eng, batch):
    """the sum of the group's signatures is unchanged: only the per-signature scalars tell.  One scalar per group, or unscaled keys, pass"""
    sig = batch["sig"].copy()
    sig[[3, 20]] = sig[[20, 3]]
    assert batch["grp_off"][1] <= 3 < 20 < batch["grp_off"][2] and batch["rows"][3] != batch["rows"][20]
    verify(eng, False, batch["pk"], batch["grp_off"], batch["msgs"], sig)


def test_a_signature_filed_under_the_wrong_group_fails(eng, batch):
    off = list(batch["grp_off"])
    off[4] += 1                                          # the first signature of group 4 moves to group 3
    verify(eng, False, batch["pk"], off, batch["msgs"], batch["sig"])
    off = list(batch["grp_off"])
    off[3] += 1                                          # ... and the first of group 3 into the group nobody signed
    verify(eng, False, batch["pk"], off, batch["msgs"], batch["sig"])


def test_an_identity_public_key_fails(eng, batch):
    pk, inf_pk = batch["pk"].copy(), np.zeros(N, dtype=np.uint8)
    sig, inf_sig = batch["sig"].copy(), np.zeros(N, dtype=np.uint8)
    pk[40], inf_pk[40] = am.g1_rows([None])[0][0], 1
    sig[40], inf_sig[40] = am.u64(h.g2_words(None)[0]), 1                # the pair the product alone would accept
    verify(eng, False, pk, batch["grp_off"], batch["msgs"], sig, inf_pk=inf_pk, inf_sig=inf_sig)


def test_a_public_key_outside_g1_with_and_without_points_checked(eng, batch):
    """a key shifted by a point of order 3: only the points check sees it - the pairing product holds as it does for the sound key
    (tests/test_gpu_bls.py states it for zkp_bls_verify_batch)"""
    _, pks = am.key_table(gm.N_TABLE)
    shifted = m.g1_add(pks[batch["rows"][50]], og.g1_points()["order3"])
    assert m.g1_on_curve(shifted) and not m.g1_torsion_free(shifted)
    pk = batch["pk"].copy()
    pk[50] = am.u64(h.g1_words(shifted)[0])
    verify(eng, False, pk, batch["grp_off"], batch["msgs"], batch["sig"])
    verify(eng, True, pk, batch["grp_off"], batch["msgs"], batch["sig"], points_checked=True)
    verify(eng, True, batch["pk"], batch["grp_off"], batch["msgs"], batch["sig"], points_checked=True)


@pytest.mark.parametrize("where", [0, 34, N - 1])
def test_a_zero_row_of_rand_fails(eng, batch, where):
    rand = gm.rand_rows(N, 31)
    rand[where] = 0
    verify(eng, False, batch["pk"], batch["grp_off"], batch["msgs"], batch["sig"], rand=rand)


def test_inf_sig_takes_a_signature_out_of_the_sum(eng, batch):
    """a flagged signature is the identity whatever its words say: the sum then lacks it and the batch fails (0), inside a group of 33 and
    as the only signature of its group; flags that are all zero change nothing (1)"""
    inf_sig = np.zeros(N, dtype=np.uint8)
    inf_sig[10] = 1
    verify(eng, False, batch["pk"], batch["grp_off"], batch["msgs"], batch["sig"], inf_sig=inf_sig)
    verify(eng, True, batch["pk"], batch["grp_off"], batch["msgs"], batch["sig"], inf_sig=np.zeros(N, dtype=np.uint8))
    inf_sig = np.zeros(N, dtype=np.uint8)
    inf_sig[0] = 1
    verify(eng, False, batch["pk"], batch["grp_off"], batch["msgs"], batch["sig"], inf_sig=inf_sig)


def test_the_empty_batch_holds_whatever_m_is(eng):
    none12, none24 = np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64)
    assert eng.bls_verify_grouped(none12, gm.off_array([0]), [], none24, DST) is True
    assert eng.bls_verify_grouped(none12, gm.off_array([0, 0, 0, 0]), [b"a", b"", b"c"], none24, DST) is True
    buf, off = pack([b"a", b"", b"c"])
    flag = eng.bls_verify_grouped(_dev(none12), _dev(gm.off_array([0, 0, 0, 0])), _dev(buf), _dev(none24), DST, offsets=_dev(off), rand=_dev(gm.rand_rows(1, 1)[:0]))
    assert int(flag.cpu().numpy()[0]) == 1
    buf, off = pack([])
    flag = eng.bls_verify_grouped(_dev(none12), _dev(gm.off_array([0])), None, _dev(none24), DST, offsets=_dev(off), rand=_dev(gm.rand_rows(1, 1)[:0]))
    assert int(flag.cpu().numpy()[0]) == 1


MALFORMED = {"decreasing": [0, 1, 40, 34, 66, 70], "first-not-zero": [1, 1, 34, 34, 66, 70], "last-beyond": [0, 1, 34, 34, 66, 71],
             "last-below": [0, 1, 34, 34, 66, 69]}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_group_offsets_give_zero_on_the_device_and_an_error_on_the_host(eng, batch, kind):
    from zkvm_pairings_amd._lib import ZkpError
    verify(eng, False, batch["pk"], MALFORMED[kind], batch["msgs"], batch["sig"], host=False, ungrouped=False)
    with pytest.raises(ZkpError) as err:
        eng.bls_verify_grouped(batch["pk"], gm.off_array(MALFORMED[kind]), batch["msgs"], batch["sig"], DST)
    assert err.value.status == -1
    verify(eng, True, batch["pk"], batch["grp_off"], batch["msgs"], batch["sig"], host=False, ungrouped=False)      # the next call is not tainted


def test_the_synthetic_instance_is_what_the_model_signs(eng):
    import zkvm_pairings_amd as z
    sizes = [2, 0, 3]
    sks, pks, msgs, grp_off, sigs = z.synthetic.bls_grouped_instance(sizes, seed=0x5EED, engine=eng)
    ints = [z.synthetic.scalar_to_int(r) for r in sks]
    assert grp_off.tolist() == [0, 2, 2, 5] and len(set(msgs)) == 3
    assert pks.tobytes() == am.table_rows([am.public_key(k) for k in ints]).tobytes()
    want = [m.g2_mul(h.hash_to_g2(x, DST), k) for x, k in zip(_expand(msgs, grp_off.tolist()), ints)]
    assert sigs.tobytes() == am.u64([h.g2_words(s)[0] for s in want]).tobytes()
    assert eng.bls_verify_grouped(pks, grp_off, msgs, sigs, DST) is True
    assert eng.bls_verify_grouped(pks, grp_off, msgs[::-1], sigs, DST) is False


# ------------------------------------------------------------------------------------------------------------------- the aggregate form
COMMITTEES = [1, 2, 33, 64, 2, 33, 1, 64, 2]            # 9 committees over 3 messages: groups of 4, 3 and 2
GROUPS = [0, 4, 7, 9]


def _aggregates():
    """nine model-signed aggregates ordered by message over am.key_table(64); committee 3 and 7 hold every key"""
    sks, pks = am.key_table(gm.N_TABLE)
    b = am.aggregate_batch(9, gm.N_TABLE, 21, sizes=COMMITTEES)
    msgs = list(am.MESSAGES[:3])
    expanded = _expand(msgs, GROUPS)
    sig = am.u64([h.g2_words(am.sign(x, sum(sks[r] for r in c)))[0] for x, c in zip(expanded, b["committees"])]).reshape(-1, 24)
    return am.table_rows(pks), b["committees"], msgs, expanded, sig


def test_aggregates_grouped_by_message_equal_the_ungrouped_call(eng):
    import zkvm_pairings_amd as z
    rows, committees, msgs, expanded, sig = _aggregates()
    rand = gm.rand_rows(9, 13)
    buf, off = pack(msgs)
    sks, _ = am.key_table(gm.N_TABLE)
    honest = sig
    for forged in (False, True):
        cs = [list(c) for c in committees]
        sig = honest.copy()
        if forged:                                       # an absent member not subtracted: the committee lists both, one signed
            sig[8] = am.u64(h.g2_words(am.sign(expanded[8], sks[cs[8][0]]))[0])
        idx, seg_off = am.entry_arrays(*am.committee_entries(cs))
        want = not forged
        flag = eng.bls_fast_aggregate_verify_grouped(_dev(rows), _dev(idx), _dev(seg_off), _dev(gm.off_array(GROUPS)), _dev(buf), _dev(sig), DST, offsets=_dev(off),
                                                     rand=_dev(rand))
        assert bool(flag.cpu().numpy()[0]) is want, "_dev flavour"
        assert eng.bls_fast_aggregate_verify_grouped(rows, idx, seg_off, gm.off_array(GROUPS), msgs, sig, DST, rand=rand) is want, "host flavour"
        assert z.bls_fast_aggregate_verify_grouped_batch(rows, cs, expanded, sig, DST, rand=rand, engine=eng) is want, "module function"
        assert z.bls_fast_aggregate_verify_batch(rows, cs, expanded, sig, DST, rand=rand, engine=eng) is want, "the ungrouped call"
    cs = [list(c) for c in committees]
    cs[4] = []                                           # an empty committee fails as it does ungrouped
    idx, seg_off = am.entry_arrays(*am.committee_entries(cs))
    assert eng.bls_fast_aggregate_verify_grouped(rows, idx, seg_off, gm.off_array(GROUPS), msgs, honest, DST, rand=rand) is False
    assert z.bls_fast_aggregate_verify_batch(rows, cs, expanded, honest, DST, rand=rand, engine=eng) is False
    none = np.zeros((0, 24), dtype=np.uint64)
    assert z.bls_fast_aggregate_verify_grouped_batch(rows, [], [], none, DST, engine=eng) is True
