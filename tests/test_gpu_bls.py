"""The BLS batch verifier on one MI355X through the C ABI (run with -m gpu).  Keys and signatures are made by the MODEL
(tests/h2c_model.py, tests/bls_replay_cases.py: a pool of model-signed messages the batches draw from), never by the library; every case
goes through both bls_verify_batch (one pairing product under a random linear combination) and bls_verify_each (per-signature flags)."""
import numpy as np
import pytest

import bls12_381_model as m
import bls_replay_cases as brc
import h2c_model as h
import outside_groups as og

pytestmark = pytest.mark.gpu
DST = h.ETH_DST
SIZES = (1, 5, 6, 61, 300)            # 5 | 6 and 60 | 61: the edges of the five-checks-per-wavefront grouping


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def verify_both(eng, b, want_all, want_each=None, msgs=None, rand=None, **kw):
    import torch
    import zkvm_pairings_amd as z
    msgs = b["msgs"] if msgs is None else msgs
    n = len(msgs)
    rand = brc.rand_rows(n, 77) if rand is None else rand
    got = z.bls_verify_batch(b["pk"], msgs, b["sig"], DST, rand=rand, engine=eng, **kw)
    assert got is want_all
    # the _dev flavour gives the same answer
    buf, off = brc.pack(msgs)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).cuda()
    kd = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    flag = eng.bls_verify(t(b["pk"]), t(buf), t(b["sig"]), DST, offsets=t(off), rand=t(rand), **kd)
    assert bool(flag.cpu().numpy()[0]) is want_all
    each = z.bls_verify_each(b["pk"], msgs, b["sig"], DST, engine=eng, **kw)
    if want_each is None:
        want_each = np.full(n, want_all)
    assert each.tolist() == list(want_each)


@pytest.mark.parametrize("n", SIZES)
def test_valid_batches_and_single_forgeries(eng, n):
    b = brc.batch(n)
    verify_both(eng, b, True)
    # one wrong message byte
    j = n - 1
    msgs = list(b["msgs"])
    msgs[j] = msgs[j][:-1] + bytes([msgs[j][-1] ^ 0x80]) if msgs[j] else b"\x00"
    each = np.ones(n, dtype=bool)
    each[j] = False
    verify_both(eng, b, False, each, msgs=msgs)
    # a public key replaced by the identity (KeyValidate)
    inf_pk = np.zeros(n, dtype=np.uint8)
    inf_pk[n // 2] = 1
    each = np.ones(n, dtype=bool)
    each[n // 2] = False
    verify_both(eng, b, False, each, inf_pk=inf_pk)


@pytest.mark.parametrize("n", [5, 61])
def test_swapped_neighbours_and_a_signature_outside_g2(eng, n):
    b = brc.batch(n)
    sw = dict(b, sig=b["sig"].copy())
    sw["sig"][[0, 1]] = b["sig"][[1, 0]]
    each = np.ones(n, dtype=bool)
    each[:2] = False
    verify_both(eng, sw, False, each)
    outside = [q for q in og.g2_points().values() if m.g2_on_curve(q) and not m.g2_torsion_free(q)]
    assert outside
    bad = dict(b, sig=b["sig"].copy())
    bad["sig"][2] = brc.u64(h.g2_words(outside[0])[0])
    each = np.ones(n, dtype=bool)
    each[2] = False
    verify_both(eng, bad, False, each)


def _down(n, *where):
    each = np.ones(n, dtype=bool)
    each[list(where)] = False
    return each


def _flags(n, *where):
    f = np.zeros(n, dtype=np.uint8)
    f[list(where)] = 1
    return f


@pytest.mark.parametrize("n", [5, 61])
def test_points_checked_skips_the_points_check_and_nothing_else(eng, n):
    b = brc.batch(n)
    verify_both(eng, b, True, points_checked=True)
    msgs = list(b["msgs"])
    msgs[1] = msgs[1] + b"!"
    verify_both(eng, b, False, _down(n, 1), msgs=msgs, points_checked=True)
    # KeyValidate is no part of the skipped check: an identity public key still refuses the batch
    for j in (0, n - 1):
        verify_both(eng, b, False, _down(n, j), inf_pk=_flags(n, j), points_checked=True)


@pytest.mark.parametrize("n", [5, 61])
def test_an_identity_signature_fails_alone_and_next_to_an_identity_key(eng, n):
    """inf_sig on a position whose stored signature is the valid one: dropping the flag would accept it.  With inf_pk on the same position
    the pairing product of that check is one, and the identity key alone refuses it"""
    b = brc.batch(n)
    for j in (0, n // 2, n - 1):
        verify_both(eng, b, False, _down(n, j), inf_sig=_flags(n, j))
    j = n // 2
    verify_both(eng, b, False, _down(n, j), inf_pk=_flags(n, j), inf_sig=_flags(n, j))


@pytest.mark.parametrize("n", [5, 61])
def test_bad_points_at_the_first_middle_and_last_position(eng, n):
    """a public key on the curve outside G1, a valid key shifted by a point of small order (the one case the pairing product cannot see: a
    verifier that skipped the points check would accept it), a public key off the curve, a signature off the curve (one outside G2: above)"""
    b = brc.batch(n)
    outside = [q for q in og.g1_points().values() if m.g1_on_curve(q) and not m.g1_torsion_free(q)]
    assert outside
    for k, j in enumerate((0, n // 2, n - 1)):
        bad = dict(b, pk=b["pk"].copy())
        bad["pk"][j] = brc.u64(h.g1_words(outside[k % len(outside)])[0])
        verify_both(eng, bad, False, _down(n, j))
        # pk + T, T of order 3 or 11: T is r times a point, so the pairing equation holds as it does for pk (the model's verify says so)
        # and only the subgroup check refuses the key
        _, pk, msg, sig = brc.signed_pool()[b["idx"][j]]
        shifted = m.g1_add(pk, og.g1_points()[("order3", "order11", "order3_neg")[k]])
        assert m.g1_on_curve(shifted) and not m.g1_torsion_free(shifted) and (n > 5 or h.verify(shifted, msg, sig, DST))
        bad["pk"][j] = brc.u64(h.g1_words(shifted)[0])
        verify_both(eng, bad, False, _down(n, j))
        off = (pk[0], (pk[1] + 1) % h.P)
        assert not m.g1_on_curve(off)
        bad["pk"][j] = brc.u64(h.g1_words(off)[0])
        verify_both(eng, bad, False, _down(n, j))
        sig = brc.signed_pool()[b["idx"][j]][3]
        off = (sig[0], (sig[1][0], (sig[1][1] + 1) % h.P))
        assert not m.g2_on_curve(off)
        bad = dict(b, sig=b["sig"].copy())
        bad["sig"][j] = brc.u64(h.g2_words(off)[0])
        verify_both(eng, bad, False, _down(n, j))


@pytest.mark.parametrize("n", [5, 61])
def test_a_zero_row_of_rand_fails_the_batch_and_half_zero_rows_do_not(eng, n):
    """(a, b) = (0, 0) would drop a check from the product: the batch is refused although every signature holds (the per-signature path
    takes no scalars: all flags up).  (a, 0) and (0, b) are non-zero exponents"""
    b = brc.batch(n)
    for j in (0, n // 2, n - 1):
        rand = brc.rand_rows(n, 31 + j)
        rand[j] = 0
        verify_both(eng, b, False, np.ones(n, dtype=bool), rand=rand)
    rand = brc.rand_rows(n, 35)
    rand[0, 1] = 0
    rand[n // 2, 0] = 0
    rand[n - 1, 1] = 0
    verify_both(eng, b, True, rand=rand)


@pytest.mark.parametrize("n", [5, 61])
def test_negated_pairs_and_duplicates(eng, n):
    b = brc.batch(n)
    pool = brc.signed_pool()
    j = n // 2
    _, pk, _, sig = pool[b["idx"][j]]
    neg = dict(b, pk=b["pk"].copy(), sig=b["sig"].copy())
    neg["pk"][j] = brc.u64(h.g1_words(m.g1_neg(pk))[0])
    neg["sig"][j] = brc.u64(h.g2_words(m.g2_neg(sig))[0])
    verify_both(eng, neg, True)                                   # e(-pk, H) e(-g1, -sig) = 1
    neg["pk"][j] = b["pk"][j]
    verify_both(eng, neg, False, _down(n, j))                     # (pk, m, -sig)
    k = b["idx"][0]
    dup = dict(pk=np.tile(b["pk"][0], (n, 1)), msgs=[pool[k][2]] * n, sig=np.tile(b["sig"][0], (n, 1)))
    verify_both(eng, dup, True)


def test_cancelling_forgeries_need_the_random_scalars(eng):
    """sig_1 + D and sig_2 - D: the plain product of the two checks is one, so equal scalars pass the batch - and random ones do not"""
    import zkvm_pairings_amd as z
    n = 6
    b = brc.batch(n)
    pool = brc.signed_pool()
    d = m.g2_mul(m.G2_GEN, 0xD1FF)
    s1, s2 = pool[b["idx"][1]][3], pool[b["idx"][2]][3]
    forged = dict(b, sig=b["sig"].copy())
    forged["sig"][1] = brc.u64(h.g2_words(m.g2_add(s1, d))[0])
    forged["sig"][2] = brc.u64(h.g2_words(m.g2_add(s2, m.g2_neg(d)))[0])
    each = np.ones(n, dtype=bool)
    each[1:3] = False
    verify_both(eng, forged, False, each)
    equal = np.tile(brc.u64([[3, 0]]), (n, 1))
    assert z.bls_verify_batch(forged["pk"], forged["msgs"], forged["sig"], DST, rand=equal, engine=eng) is True
    assert z.bls_verify_batch(forged["pk"], forged["msgs"], forged["sig"], DST, engine=eng) is False      # fresh scalars from the OS


def test_sign_round_trip_compressed_inputs_and_the_empty_batch(eng):
    import zkvm_pairings_amd as z
    pool = brc.signed_pool()[:5]
    sks = brc.u64([[(sk >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for sk, _, _, _ in pool])
    msgs = [x[2] for x in pool]
    sig, inf = z.bls_sign_batch(sks, msgs, DST, engine=eng)
    want, winf = brc.point_rows([x[3] for x in pool])
    assert inf.tobytes() == winf.tobytes() and sig.tobytes() == want.tobytes()
    pk = brc.u64([h.g1_words(x[1])[0] for x in pool])
    pkb, sgb = eng.compress_points(pk, 1), eng.compress_points(sig, 2)
    assert z.bls_verify_batch_compressed(pkb, msgs, sgb, DST, engine=eng) is True
    assert z.bls_verify_each_compressed(pkb, msgs, sgb, DST, engine=eng).tolist() == [True] * 5
    rot = msgs[1:] + msgs[:1]
    assert z.bls_verify_batch_compressed(pkb, rot, sgb, DST, engine=eng) is False
    sks2, pks2, msgs2, sigs2 = z.synthetic.bls_instance(7, engine=eng)
    assert z.bls_verify_batch(pks2, msgs2, sigs2, DST, engine=eng) is True
    assert z.bls_verify_batch(np.zeros((0, 12), dtype=np.uint64), [], np.zeros((0, 24), dtype=np.uint64), DST, engine=eng) is True
    # argument errors of the verifier: an unknown flag, a tag of 256 bytes
    import ctypes
    ok = ctypes.c_int(5)
    buf, off = brc.pack(msgs)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    r = brc.rand_rows(5, 1)
    d = np.frombuffer(DST, dtype=np.uint8)
    assert eng._lib.zkp_bls_verify_batch(eng._h, p(pk), None, p(buf), p(off), p(d), d.size, p(sig), None, 5, p(r), 2, ctypes.byref(ok)) == -1
    assert eng._lib.zkp_bls_verify_batch(eng._h, p(pk), None, p(buf), p(off), p(d), 256, p(sig), None, 5, p(r), 0, ctypes.byref(ok)) == -1
    assert eng._lib.zkp_bls_verify_batch(eng._h, p(pk), None, p(buf), p(off), p(d), d.size, p(sig), None, (1 << 24) + 1, p(r), 0, ctypes.byref(ok)) == -1
    assert ok.value == 5
