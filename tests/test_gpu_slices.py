"""The slice loops of the G1 NTT, FK20 (csrc/zkp_fk20.hip), the KZG opening (csrc/zkp_poly.hip) and of hash-to-G2 and the BLS verifier
(csrc/zkp_bls.hip), of hash-to-G1 and the min-sig verifiers (csrc/zkp_bls_minsig.hip), and the grouped and the committee verifier above
2^17 messages or committees, on one MI355X (run with -m gpu): every
call here is the smallest that crosses a slice boundary of its entry point and ends in a short last slice, its inputs and expected bytes
are assembled from a small pool by a pseudo-random index sequence (tests/slice_pools.py), and tests/test_slices_cpu.py has shown without
a GPU that a slice which took offset 0, the previous slice's offset, or another slice's rows in ANY operand cannot give these bytes.
Every comparison is byte for byte; a failure names the first wrong item, its slice and its place in the slice."""
import numpy as np
import pytest

import fk20_replay_cases as frc
import poly_model as pm
import replay_cases as rc
import slice_pools as sp
from replay_cases import fr_rows

pytestmark = pytest.mark.gpu
R = pm.R


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    """makes the verifier's setup; never the engine under test"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def to_host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.ascontiguousarray(t)


def same(call, got, what):
    """got: name -> array or tensor, for every expected output of the call"""
    assert set(got) == set(call.outputs), what
    for name, (want, per) in call.outputs.items():
        g = to_host(got[name])
        assert g.nbytes == want.nbytes, (what, name, g.shape, want.shape)
        g = g.view(want.dtype).reshape(want.shape)
        if g.tobytes() != want.tobytes():
            pytest.fail("%s: output %s differs, first at %r" % (what, name, sp.first_difference(g, want, per, call)))


# ------------------------------------------------------------------------------------------------------------------- the G1 NTT
@pytest.mark.parametrize("flags", [0, pm.INVERSE | pm.BITREV])
def test_g1_ntt_three_slices_of_different_vectors(eng, flags):
    """N = 8, 2 * 32768 + 5 vectors: flags 0 loads bit-reversed and stores natural, INVERSE | BITREV loads and stores natural and scales.
    The host flavour out of place, the device flavour in place over points and flags"""
    call = sp.ntt_call(flags)
    inverse, bitrev = bool(flags & pm.INVERSE), bool(flags & pm.BITREV)
    pts, inf = call.arg("points"), call.arg("inf")
    assert inf.any()
    out, out_inf = eng.g1_ntt(pts, sp.NTT_LOG2, inverse=inverse, bitrev=bitrev, inf=inf)
    same(call, dict(out=out, out_inf=out_inf), "g1_ntt flags %d (host)" % flags)
    tp, ti = to_dev(pts), to_dev(inf)
    to, toi = eng.g1_ntt(tp, sp.NTT_LOG2, inverse=inverse, bitrev=bitrev, inf=ti, out=tp, out_inf=ti)
    assert to is tp and toi is ti
    same(call, dict(out=to, out_inf=toi), "g1_ntt flags %d (dev, in place)" % flags)


def test_g1_ntt_three_slices_without_input_flags(eng):
    """inf = NULL across two boundaries, on vectors that differ from slice to slice (no identity entry in any input)"""
    call = sp.ntt_call(0, finite=True)
    assert not call.arg("inf").any()
    to, toi = eng.g1_ntt(to_dev(call.arg("points")), sp.NTT_LOG2)
    same(call, dict(out=to, out_inf=toi), "g1_ntt inf = None (dev)")


# ------------------------------------------------------------------------------------------------------------------- FK20
@pytest.mark.parametrize("bitrev", [False, True])
def test_fk20_two_slices_of_different_polynomials(eng, bitrev):
    """N = 4, 32768 + 3 polynomials: the coefficient, proof and flag offsets of the second slice, whose three polynomials (a constant one
    among them) occur nowhere in the first"""
    call = sp.fk20_call(bitrev)
    setup, sinf = frc.fk20_setup_for(sp.FK20_LOG2)
    coeffs = call.arg("coeffs")
    proof, inf = eng.kzg_fk20(setup, sinf, coeffs, sp.FK20_LOG2, bitrev)
    same(call, dict(proof=proof, inf=inf), "kzg_fk20 bitrev %d (host)" % bitrev)
    tp, ti = eng.kzg_fk20(to_dev(setup), to_dev(sinf), to_dev(coeffs), sp.FK20_LOG2, bitrev)
    same(call, dict(proof=tp, inf=ti), "kzg_fk20 bitrev %d (dev)" % bitrev)


# ------------------------------------------------------------------------------------------------------------------- the opening
@pytest.mark.parametrize("bitrev", [False, True])
def test_kzg_open_two_slices_with_a_short_last_one(eng, helper, bitrev):
    """N = 2^10, 4096 + 3 openings: the last slice has its own EvalLayout (another `den` offset, one sum block).  The device flavour on
    both orders, the host flavour on the bit-reversed one; the verifier on the three proofs of the tail"""
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import synthetic
    call = sp.open_call(bitrev)
    p = call.pool
    lag, evals, zs = p["setup"].lagrange_g1, call.arg("evals"), call.arg("z")
    ty, tp, ti = eng.kzg_open(to_dev(lag), to_dev(evals), to_dev(zs), sp.OPEN_LOG2, bitrev)
    same(call, dict(y=ty, proof=tp, inf=ti), "kzg_open bitrev %d (dev)" % bitrev)
    y, proof, inf = to_host(ty), to_host(tp).view(np.uint64), to_host(ti)
    if bitrev:
        y, proof, inf = eng.kzg_open(lag, evals, zs, sp.OPEN_LOG2, bitrev)
        same(call, dict(y=y, proof=proof, inf=inf), "kzg_open bitrev %d (host)" % bitrev)
    # what the last slice produced, against commitments made from the same trapdoor
    t = slice(call.n - call.tail, call.n)
    ids = list(sp.OPEN_TAIL)
    vs = z.KzgSetup(synthetic.G1_GENERATOR, synthetic.G2_GENERATOR, rc._g2(helper, [sp.TAU])[0])
    c, cinf = p["commit"][ids], p["cinf"][ids]
    y_t = np.ascontiguousarray(y.view(np.uint64).reshape(-1, 4)[t])
    args = dict(engine=helper, inf_c=cinf, inf_proof=np.ascontiguousarray(inf[t]))
    assert z.kzg_verify_batch(vs, c, zs[t], y_t, np.ascontiguousarray(proof.reshape(-1, 12)[t]), **args) is True
    y_bad = fr_rows([(int.from_bytes(y_t[k].tobytes(), "little") + (k == 2)) % R for k in range(3)])
    assert z.kzg_verify_batch(vs, c, zs[t], y_bad, np.ascontiguousarray(proof.reshape(-1, 12)[t]), **args) is False


# ------------------------------------------------------------------------------------------------------------------- hash-to-G2 and the BLS verifier
@pytest.mark.parametrize("points", [False, True])
def test_hash_two_slices_of_mixed_length_messages(eng, points):
    """2^17 + 61 messages of 0 .. 120 bytes behind a non-zero offsets[0]: k_h2f's message index and output pointer in the second slice, whose
    four messages occur nowhere in the first; for hash_to_g2 also the u values and projective points of a slice written over the previous
    slice's, and a last launch of k_h2c_clear with one full and one partial wavefront"""
    import h2c_model as h
    call = sp.hash_call(points)
    name = "hash_to_g2" if points else "hash_to_field_g2"
    keys = ("points", "inf") if points else ("u",)
    got = getattr(eng, name)(call.msgs, h.ETH_DST, offsets=call.offsets)
    same(call, dict(zip(keys, got if points else (got,))), name + " (host)")
    got = getattr(eng, name)(to_dev(call.msgs), h.ETH_DST, offsets=to_dev(call.offsets))
    same(call, dict(zip(keys, got if points else (got,))), name + " (dev)")


def test_map_three_slices_with_an_identity_in_the_tail(eng):
    """2 * 2^17 + 5 pairs of field elements: the input and output pointers of the second and third slice; (a, -a) among the five of the tail"""
    call = sp.map_call()
    assert call.want("inf")[call.n - call.tail:].any()
    pts, inf = eng.g2_map_from_fields(call.arg("u"))
    same(call, dict(points=pts, inf=inf), "g2_map_from_fields (host)")
    pts, inf = eng.g2_map_from_fields(to_dev(call.arg("u")))
    same(call, dict(points=pts, inf=inf), "g2_map_from_fields (dev)")


def _verify(eng, call, msgs, dev):
    import h2c_model as h
    t = to_dev if dev else (lambda a: a)
    got = eng.bls_verify(t(call.arg("pk")), t(msgs), t(call.arg("sig")), h.ETH_DST, offsets=t(call.offsets), rand=t(call.arg("rand")))
    return bool(to_host(got)[0]) if dev else got


def test_bls_verify_two_slices_holds(eng):
    """2^17 + 6 model-signed messages: the hashed point of every check of the second slice must be its own for the product to be one"""
    call = sp.verify_call()
    assert _verify(eng, call, call.msgs, False) is True
    assert _verify(eng, call, call.msgs, True) is True


@pytest.mark.parametrize("where", [0, 1, 2])
def test_bls_verify_one_forgery_on_either_side_of_the_boundary(eng, where):
    """one message byte changed in the last item of the first slice, the first of the second, or the last of the call: the batch fails and
    bls_verify_each names exactly that signature"""
    import h2c_model as h
    import zkvm_pairings_amd as z
    call = sp.verify_call()
    j = call.forged[where]
    bad = sp.forged_messages(call, j)
    assert _verify(eng, call, bad, False) is False
    assert _verify(eng, call, bad, True) is False
    each = z.bls_verify_each(call.arg("pk"), sp.message_list(call, bad), call.arg("sig"), h.ETH_DST, engine=eng)
    assert np.nonzero(~each)[0].tolist() == [j]


# ------------------------------------------------------------------------------------------------------------------- hash-to-G1 and the min-sig verifiers
def _minsig_dst():
    import h2g1_model as g
    return g.QUICKNET_DST


def test_hash_to_field_g1_two_slices_of_mixed_length_messages(eng):
    """2^17 + 61 messages behind a non-zero offsets[0]: g1h_field_dev's output pointer and k_g1h_field's message index in the second slice"""
    call = sp.minsig_field_call()
    got = eng.hash_to_field_g1(call.msgs, _minsig_dst(), offsets=call.offsets)
    same(call, dict(u=got), "hash_to_field_g1 (host)")
    got = eng.hash_to_field_g1(to_dev(call.msgs), _minsig_dst(), offsets=to_dev(call.offsets))
    same(call, dict(u=got), "hash_to_field_g1 (dev)")


def test_g1_map_three_slices_with_an_identity_in_the_tail(eng):
    """2 * 2^17 + 5 pairs of field elements: g1h_map_dev's input and output pointers in the second and third slice; (a, -a) in the tail"""
    call = sp.minsig_map_call()
    assert call.want("inf")[call.n - call.tail:].any()
    pts, inf = eng.g1_map_from_fields(call.arg("u"))
    same(call, dict(points=pts, inf=inf), "g1_map_from_fields (host)")
    pts, inf = eng.g1_map_from_fields(to_dev(call.arg("u")))
    same(call, dict(points=pts, inf=inf), "g1_map_from_fields (dev)")


@pytest.mark.parametrize("flags", [True, False], ids=["inf", "inf-none"])
def test_g1_clear_cofactor_three_slices_of_points_of_every_kind(eng, flags):
    """2 * 2^17 + 5 points of E, identities of every kind among them: g1h_clear_dev's point, flag and output pointers in every slice.
    Without the flag bytes the rows whose input is a flagged identity are compared with nothing: their words are then a point off the curve"""
    call = sp.minsig_clear_call()
    pin, iin = call.arg("pts"), call.arg("inf")
    if flags:
        pts, inf = eng.g1_clear_cofactor(pin, iin)
        same(call, dict(points=pts, inf=inf), "g1_clear_cofactor (host)")
        pts, inf = eng.g1_clear_cofactor(to_dev(pin), to_dev(iin))
        same(call, dict(points=pts, inf=inf), "g1_clear_cofactor (dev)")
        return
    keep = iin == 0
    for what, got in (("host", eng.g1_clear_cofactor(pin)), ("dev", eng.g1_clear_cofactor(to_dev(pin)))):
        for name, g in zip(("points", "inf"), got):
            want = call.want(name)
            g = to_host(g).view(want.dtype).reshape(want.shape).copy()
            g[~keep] = want[~keep]
            if g.tobytes() != want.tobytes():
                pytest.fail("g1_clear_cofactor inf = None (%s): output %s differs, first at %r" % (what, name, sp.first_difference(g, want, 1, call)))


_RESIDENT = {}


def _resident(key, build):
    """the device tensors of a call, made once for the tests that share it"""
    if key not in _RESIDENT:
        _RESIDENT[key] = build()
    return _RESIDENT[key]


def _minsig_verify(eng, same_key, msgs=None, sig=None, inf_pk=None):
    call = sp.minsig_verify_call(same_key)
    t = _resident(("minsig", same_key), lambda: dict(pk=to_dev(call.pk1 if same_key else call.arg("pk")), msgs=to_dev(call.msgs), sig=to_dev(call.arg("sig")),
                                                     off=to_dev(call.offsets), rand=to_dev(call.arg("rand"))))
    msgs = t["msgs"] if msgs is None else to_dev(msgs)
    sig = t["sig"] if sig is None else to_dev(sig)
    if same_key:
        ok = eng.bls_minsig_verify_samekey(t["pk"], msgs, sig, _minsig_dst(), offsets=t["off"], rand=t["rand"])
    else:
        ok = eng.bls_minsig_verify(t["pk"], msgs, sig, _minsig_dst(), offsets=t["off"], rand=t["rand"], inf_pk=None if inf_pk is None else to_dev(inf_pk))
    return bool(to_host(ok)[0])


@pytest.mark.parametrize("same_key", [False, True], ids=["general", "samekey"])
def test_minsig_verify_two_slices_holds(eng, same_key):
    """2^17 + 6 model-signed messages: hash_into's output pointer, hp + 12 at ostride (ostride 2 for the same-key rows), must be the slice's own"""
    assert _minsig_verify(eng, same_key) is True


@pytest.mark.parametrize("where", [0, 1, 2])
@pytest.mark.parametrize("same_key", [False, True], ids=["general", "samekey"])
def test_minsig_verify_one_forgery_on_either_side_of_the_boundary(eng, same_key, where):
    call = sp.minsig_verify_call(same_key)
    assert _minsig_verify(eng, same_key, msgs=sp.forged_messages(call, call.forged[where])) is False


@pytest.mark.parametrize("same_key", [False, True], ids=["general", "samekey"])
def test_minsig_verify_a_signature_outside_g1_behind_the_boundary(eng, same_key):
    """signature 2^17 + 2 moved by a point of order 3: the product still holds, only the status byte st[n + 2^17 + 2] (same key: st[2^17 + 2])
    refuses the batch"""
    call = sp.minsig_verify_call(same_key)
    assert _minsig_verify(eng, same_key, sig=sp.shifted_signature(call, call.shifted)[0]) is False


def test_minsig_verify_an_identity_key_behind_the_boundary(eng):
    call = sp.minsig_verify_call(False)
    inf_pk = np.zeros(call.n, dtype=np.uint8)
    assert _minsig_verify(eng, False, inf_pk=inf_pk) is True                                   # flags that are all zero change nothing
    inf_pk[call.flagged_pk] = 1
    assert _minsig_verify(eng, False, inf_pk=inf_pk) is False


# ------------------------------------------------------------------------------------------------------------------- committees and groups above 2^17
def _i32(a):
    return to_dev(np.ascontiguousarray(a).view(np.int32))


def _committees():
    call = sp.committees_call()
    t = _resident("committees", lambda: dict(table=to_dev(call.pool["table"]), entries=_i32(call.entries), seg_off=to_dev(call.seg_off), msgs=to_dev(call.msgs),
                                             off=to_dev(call.offsets), sig=to_dev(call.arg("sig")), rand=to_dev(call.arg("rand"))))
    return call, t


def test_g1_segment_sum_on_two_to_the_17_and_six_committees(eng):
    """2^17 + 6 segments of 1 .. 33 signed table rows, about 10^6 entries: k_agg_keys' search and k_agg_affine beyond a few hundred segments"""
    call, t = _committees()
    out, oi, st = eng.g1_segment_sum(t["table"], t["entries"], t["seg_off"])
    want = call.want("apk")
    g = to_host(out).view(np.uint64).reshape(want.shape)
    if g.tobytes() != want.tobytes():
        pytest.fail("g1_segment_sum: out differs, first at %r" % sp.first_difference(g, want, 1, call))
    assert not to_host(oi).any() and not to_host(st).any() and to_host(oi).shape == to_host(st).shape == (call.n,)


def _aggregate_verify(eng, entries=None):
    import h2c_model as h
    call, t = _committees()
    ok = eng.bls_fast_aggregate_verify(t["table"], t["entries"] if entries is None else _i32(entries), t["seg_off"], t["msgs"], t["sig"], h.ETH_DST, offsets=t["off"],
                                       rand=t["rand"])
    return bool(to_host(ok)[0])


def test_fast_aggregate_verify_two_slices_of_committees_holds(eng):
    """bls_verify_dev on 2^17 + 6 aggregate keys held in the workspace: every slice of it must take its own keys, flags and hashed points"""
    assert _aggregate_verify(eng) is True


@pytest.mark.parametrize("where", [0, 1, 2])
def test_fast_aggregate_verify_one_wrong_member_on_either_side_of_the_boundary(eng, where):
    call = sp.committees_call()
    assert _aggregate_verify(eng, sp.swapped_member(call, call.forged[where])[0]) is False


def _grouped(eng, msgs=None, grp_off=None, expanded=False):
    """bls_verify_grouped, or bls_verify on the messages expanded per signature, with the same rand"""
    import h2c_model as h
    call = sp.grouped_call()
    t = _resident("grouped", lambda: dict(pk=to_dev(call.pk), sig=to_dev(call.sig), rand=to_dev(call.rand), grp_off=to_dev(call.grp_off), msgs=to_dev(call.msgs),
                                          off=to_dev(call.offsets)))
    if expanded:
        buf, off = sp.expanded_messages(call, msgs)
        ok = eng.bls_verify(t["pk"], to_dev(buf), t["sig"], h.ETH_DST, offsets=to_dev(off), rand=t["rand"])
    else:
        ok = eng.bls_verify_grouped(t["pk"], t["grp_off"] if grp_off is None else to_dev(grp_off), t["msgs"] if msgs is None else to_dev(msgs), t["sig"], h.ETH_DST,
                                    offsets=t["off"], rand=t["rand"])
    return bool(to_host(ok)[0])


def test_verify_grouped_two_slices_of_messages_holds_as_the_ungrouped_call_does(eng):
    """2^17 + 6 messages, one signature more: h2c_hash_dev over m messages in two slices, k_grp_keys and k_grp_affine over 2^17 + 6 groups,
    a Miller product of m pairs; groups of 0, 2 and 3 signatures at 5, 6, 2^17 - 2 and 2^17"""
    assert _grouped(eng) is True
    assert _grouped(eng, expanded=True) is True


@pytest.mark.parametrize("where", [0, 1, 2])
def test_verify_grouped_one_changed_message_on_either_side_of_the_boundary(eng, where):
    call = sp.grouped_call()
    bad = sp.forged_messages(call, call.forged[where])
    assert _grouped(eng, msgs=bad) is False
    if where == 1:
        assert _grouped(eng, msgs=bad, expanded=True) is False


def test_verify_grouped_a_signature_filed_under_its_neighbour_behind_the_boundary(eng):
    call = sp.grouped_call()
    off = call.grp_off.copy()
    off[call.moved] += 1
    assert _grouped(eng, grp_off=off) is False
