"""FastAggregateVerify for committees of G2 keys (the minimal-signature-size layout) on one MI355X through the C ABI (run with -m gpu):
the cases of tests/test_gpu_bls_aggregate.py.  The key table (64 keys [sk] g2), the committees and the aggregate signatures in G1 are made
by the MODEL (tests/agg_g2_model.py: [sum of the members' secret keys] H(m) through tests/h2g1_model.py), never by the library; every
case goes through bls_minsig_fast_aggregate_verify_batch in the host and the _dev flavour and through
bls_minsig_fast_aggregate_verify_each (per-aggregate flags)."""
import numpy as np
import pytest

import agg_g2_model as a2
import agg_model as am
import bls12_381_model as m
import h2c_model as h
import h2g1_model as g
import outside_groups as og
from test_gpu_bls_aggregate import SIZES, _dev, _down

pytestmark = pytest.mark.gpu
DST = a2.MINSIG_DST
N_TABLE = 64


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys():
    """(secret keys, model points, rows (64, 24))"""
    sks, pks = a2.minsig_key_table(N_TABLE)
    return sks, pks, a2.g2_rows(pks)[0]


def _batch(n):
    return a2.minsig_aggregate_batch(n, N_TABLE, 1, sizes=SIZES[n])


def verify_all(eng, rows, idx, seg_off, msgs, sig, want_all, want_each=None, rand=None, host=True, **kw):
    """idx, seg_off: lists.  The _dev flavour, then (unless the host flavour refuses such input) the host flavour and the per-aggregate path"""
    import zkvm_pairings_amd as z
    from bls_replay_cases import pack
    n = len(msgs)
    a_idx, a_off = am.entry_arrays(idx, seg_off)
    rand = am.rand_rows(n, 77) if rand is None else rand
    buf, off = pack(msgs)
    kd = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    flag = eng.bls_minsig_fast_aggregate_verify(_dev(rows), _dev(a_idx), _dev(a_off), _dev(buf), _dev(sig), DST, offsets=_dev(off), rand=_dev(rand), **kd)
    assert bool(flag.cpu().numpy()[0]) is want_all, "_dev flavour"
    if not host:
        return
    assert z.bls_minsig_fast_aggregate_verify_batch(rows, (a_idx, a_off), msgs, sig, DST, rand=rand, engine=eng, **kw) is want_all, "host flavour"
    each = z.bls_minsig_fast_aggregate_verify_each(rows, (a_idx, a_off), msgs, sig, DST, engine=eng, **kw)
    assert each.tolist() == list(np.full(n, want_all) if want_each is None else want_each)


@pytest.mark.parametrize("n", [1, 5, 65])
def test_model_signed_aggregates_verify_as_bls_minsig_verify_does_on_model_summed_keys(eng, keys, n):
    import zkvm_pairings_amd as z
    _, pks, rows = keys
    b = _batch(n)
    assert n != 65 or sorted(set(len(c) for c in b["committees"])) == list(range(1, 41))
    idx, seg_off = am.committee_entries(b["committees"])
    verify_all(eng, rows, idx, seg_off, b["msgs"], b["sig"], True)
    assert z.bls_minsig_fast_aggregate_verify_batch(rows, b["committees"], b["msgs"], b["sig"], DST, rand=am.rand_rows(n, 5), engine=eng) is True
    apk, inf = a2.g2_rows(a2.segment_sums(pks, idx, seg_off)[0])
    assert not inf.any()
    assert z.bls_minsig_verify_batch(apk, b["msgs"], b["sig"], DST, rand=am.rand_rows(n, 5), engine=eng) is True          # the second witness
    got, ginf = z.bls_minsig_aggregate_keys(rows, b["committees"], engine=eng)
    assert got.tobytes() == apk.tobytes() and not ginf.any()


FORGERIES = ("replaced", "dropped", "duplicated", "sign-flipped", "other-message")


@pytest.mark.parametrize("kind", FORGERIES)
def test_one_forged_aggregate_at_the_first_a_middle_and_the_last_committee(eng, keys, kind):
    sks, _, rows = keys
    n = 5
    b = _batch(n)
    for j in (0, 2, n - 1):
        committees = [list(c) for c in b["committees"]]
        sig = b["sig"]
        c = committees[j]
        if kind == "replaced":
            c[1] = next(r for r in range(N_TABLE) if r not in c)
        elif kind == "dropped":
            del c[1]
        elif kind == "duplicated":
            c.append(c[0])
        elif kind == "sign-flipped":
            c[-1] |= am.SIGN
        else:
            other = am.MESSAGES[(j + 4) % len(am.MESSAGES)]
            assert other != b["msgs"][j]
            sig = sig.copy()
            sig[j] = am.u64(h.g1_words(a2.minsig_sign(other, sum(sks[r] for r in c)))[0])
        idx, seg_off = am.committee_entries(committees)
        verify_all(eng, rows, idx, seg_off, b["msgs"], sig, False, _down(n, j))


def test_an_empty_committee_a_cancelling_committee_and_a_row_beyond_the_table_fail(eng, keys):
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd._lib import ZkpError
    _, _, rows = keys
    n = 5
    b = _batch(n)
    for j in (0, 2, n - 1):
        committees = [list(c) for c in b["committees"]]
        committees[j] = []
        idx, seg_off = am.committee_entries(committees)
        verify_all(eng, rows, idx, seg_off, b["msgs"], b["sig"], False, _down(n, j))
        # ... also with the signature the identity, which the pairing product of an identity key would accept
        sig, inf_sig = b["sig"].copy(), np.zeros(n, dtype=np.uint8)
        sig[j], inf_sig[j] = am.u64(h.g1_words(None)[0]), 1
        verify_all(eng, rows, idx, seg_off, b["msgs"], sig, False, _down(n, j), inf_sig=inf_sig)
        committees[j] = [9, 9 | am.SIGN]                                  # +a - a: the aggregate is the identity (KeyValidate)
        idx, seg_off = am.committee_entries(committees)
        verify_all(eng, rows, idx, seg_off, b["msgs"], sig, False, _down(n, j), inf_sig=inf_sig)
        committees[j] = list(b["committees"][j]) + [N_TABLE]              # a row beyond the table: the _dev flavour answers 0 ...
        idx, seg_off = am.committee_entries(committees)
        verify_all(eng, rows, idx, seg_off, b["msgs"], b["sig"], False, host=False)
        with pytest.raises(ZkpError) as err:                              # ... and the host flavour refuses the call
            z.bls_minsig_fast_aggregate_verify_batch(rows, am.entry_arrays(idx, seg_off), b["msgs"], b["sig"], DST, engine=eng)
        assert err.value.status == -1
    idx, bad_off = am.committee_entries(b["committees"])
    bad_off[-1] += 1                                                      # the last offset beyond the entries: the call is malformed
    verify_all(eng, rows, idx, bad_off, b["msgs"], b["sig"], False, host=False)


def test_points_checked_skips_the_check_of_the_aggregates_and_nothing_else(eng, keys):
    """a table row shifted by a point of order 13 of the twist: every aggregate that holds it leaves G2 and the points check refuses
    exactly those committees.  What the pairing makes of a G2 argument outside the subgroup is no statement of the scheme, so the verdict
    on that table with points_checked is not asserted; that the flag skips the check of the SIGNATURES is shown on a signature moved by
    (0, 2), a point of order 3 of E, which the pairing product cannot see (tests/test_gpu_bls_minsig.py states it for single signatures).
    An empty committee, a cancelling one and a row beyond the table are no part of the skipped check."""
    _, pks, rows = keys
    n = 5
    b = _batch(n)
    row = b["committees"][0][0]
    shifted = m.g2_add(pks[row], og.g2_points()["order13"])
    assert m.g2_on_curve(shifted) and not m.g2_torsion_free(shifted)
    bad_rows = rows.copy()
    bad_rows[row] = am.u64(h.g2_words(shifted)[0])
    hit = [j for j, c in enumerate(b["committees"]) if row in c]
    assert 0 in hit and len(hit) < n
    idx, seg_off = am.committee_entries(b["committees"])
    verify_all(eng, bad_rows, idx, seg_off, b["msgs"], b["sig"], False, _down(n, *hit))
    verify_all(eng, rows, idx, seg_off, b["msgs"], b["sig"], True, points_checked=True)
    moved = b["sig"].copy()
    pt = g.words_g1(b["sig"][1].tolist(), 0)
    moved[1] = am.u64(h.g1_words(g.e_add(pt, (0, 2)))[0])
    verify_all(eng, rows, idx, seg_off, b["msgs"], moved, False, _down(n, 1))
    verify_all(eng, rows, idx, seg_off, b["msgs"], moved, True, points_checked=True)
    committees = [list(c) for c in b["committees"]]
    committees[n - 1] = []
    idx2, off2 = am.committee_entries(committees)
    verify_all(eng, rows, idx2, off2, b["msgs"], b["sig"], False, _down(n, n - 1), points_checked=True)
    committees[n - 1] = [9, 9 | am.SIGN]
    idx2, off2 = am.committee_entries(committees)
    verify_all(eng, rows, idx2, off2, b["msgs"], b["sig"], False, _down(n, n - 1), points_checked=True)
    committees[n - 1] = list(b["committees"][n - 1]) + [N_TABLE]
    idx2, off2 = am.committee_entries(committees)
    verify_all(eng, rows, idx2, off2, b["msgs"], b["sig"], False, host=False, points_checked=True)


def test_a_zero_row_of_rand_fails_and_the_empty_batch_holds(eng, keys):
    import zkvm_pairings_amd as z
    _, _, rows = keys
    n = 5
    b = _batch(n)
    idx, seg_off = am.committee_entries(b["committees"])
    for j in (0, 2, n - 1):
        rand = am.rand_rows(n, 31 + j)
        rand[j] = 0
        verify_all(eng, rows, idx, seg_off, b["msgs"], b["sig"], False, np.ones(n, dtype=bool), rand=rand)
    none = np.zeros((0, 12), dtype=np.uint64)
    assert z.bls_minsig_fast_aggregate_verify_batch(rows, [], [], none, DST, engine=eng) is True
    assert z.bls_minsig_fast_aggregate_verify_each(rows, [], [], none, DST, engine=eng).tolist() == []
    verify_all(eng, rows, [], [0], [], none, True, host=False)


def test_the_synthetic_instance_is_what_the_model_signs(eng, keys):
    import zkvm_pairings_amd as z
    sizes = [1, 7, 40, 2]
    sks, table, committees, msgs, sigs = z.synthetic.bls_minsig_aggregate_instance(16, sizes, seed=0x5EED, engine=eng, dst=DST)
    ints = [z.synthetic.scalar_to_int(r) for r in sks]
    assert [len(c) for c in committees] == sizes and all(0 <= r < 16 for c in committees for r in c)
    assert table.tobytes() == a2.g2_rows([a2.minsig_public_key(k) for k in ints])[0].tobytes()
    want = [a2.minsig_sign(x, sum(ints[r] for r in c)) for x, c in zip(msgs, committees)]
    assert sigs.tobytes() == am.u64([h.g1_words(s)[0] for s in want]).tobytes()
    assert z.bls_minsig_fast_aggregate_verify_batch(table, committees, msgs, sigs, DST, engine=eng) is True
    assert z.bls_minsig_fast_aggregate_verify_each(table, committees, msgs, sigs, DST, engine=eng).tolist() == [True] * 4
    assert z.bls_minsig_fast_aggregate_verify_batch(table, committees[1:] + committees[:1], msgs, sigs, DST, engine=eng) is False
