"""CPU gate for tests/test_gpu_slices.py: the conditions under which a byte comparison of a sliced call proves that every slice took its
own offsets (the docstring of tests/slice_pools.py states them).  The slice lengths the GPU tests assume are what the planning headers
compute for the exact shapes; every shape crosses its boundaries and ends in a short slice; no slice of any input or expected output
equals another slice's rows; the expected arrays read with a wrong offset differ from the true ones in every output array; the pools
are consistent on integers by a second route.  The same for the sliced calls of csrc/zkp_bls.hip: hash_to_field_g2, hash_to_g2, the map
and the verifier (BLS_NAMES), for those of csrc/zkp_bls_minsig.hip (MINSIG_NAMES) and for the grouped and the committee verifier above
2^17 messages or committees (DRIVER_NAMES).  No GPU and no library call."""
import os
import subprocess

import numpy as np
import pytest

import fk20_model as fm
import poly_model as pm
import poly_replay_cases as prc
import slice_pools as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
R = pm.R
NTT_FLAGS = (0, pm.INVERSE | pm.BITREV)

PROGRAM = """
#include <cstdio>
#include "zkp_fk20_plan.hpp"
#include "zkp_poly_plan.hpp"
#include "zkp_bls_plan.hpp"
#include "zkp_bls_minsig_plan.hpp"
int main() {
    using namespace zkp;
    std::printf("g1ntt %%zu\\n", fk20::slice_vectors((size_t)%d, %du));
    std::printf("fk20 %%zu\\n", fk20::fk20_layout((size_t)%d, %du).slice);
    std::printf("open %%zu\\n", poly::open_slice((size_t)%d, %du));
    std::printf("g1ntt_max %%zu\\n", fk20::slice_vectors((size_t)4, fk20::G1NTT_MAX_LOG2));
    std::printf("fk20_max %%zu\\n", fk20::fk20_layout((size_t)4, fk20::FK20_MAX_LOG2).slice);
    std::printf("open_max %%zu\\n", poly::open_slice((size_t)16, poly::NTT_MAX_LOG2));
    std::printf("bls_const %%zu\\n", bls::SLICE);
    std::printf("bls_hash %%zu\\n", bls::layout((size_t)%d, false).slice);
    std::printf("bls_map %%zu\\n", bls::layout((size_t)%d, false).slice);
    std::printf("bls_verify %%zu\\n", bls::layout((size_t)%d, true).slice);
    std::printf("bls_small %%zu\\n", bls::layout((size_t)5, true).slice);
    std::printf("bls_stride %%zu\\n", (bls::layout((size_t)%d, false).hq - bls::layout((size_t)%d, false).pts) / (bls::POINT_I32 * 4));
    std::printf("minsig_const %%zu\\n", minsig::SLICE);
    std::printf("minsig_field %%zu\\n", minsig::layout((size_t)%d, minsig::HASH).slice);
    std::printf("minsig_map %%zu\\n", minsig::layout((size_t)%d, minsig::HASH).slice);
    std::printf("minsig_clear %%zu\\n", minsig::layout((size_t)%d, minsig::HASH).slice);
    std::printf("minsig_verify %%zu\\n", minsig::layout((size_t)%d, minsig::VERIFY).slice);
    std::printf("minsig_samekey %%zu\\n", minsig::layout((size_t)%d, minsig::SAMEKEY).slice);
    std::printf("minsig_small %%zu %%zu %%zu\\n", minsig::layout((size_t)5, minsig::HASH).slice, minsig::layout((size_t)5, minsig::VERIFY).slice,
                minsig::layout((size_t)5, minsig::SAMEKEY).slice);
    std::printf("bls_grouped %%zu\\n", bls::layout((size_t)%d, false).slice);
    std::printf("bls_committees %%zu\\n", bls::layout((size_t)%d, true).slice);
    return 0;
}
"""


@pytest.fixture(scope="module")
def header_slices(tmp_path_factory):
    d = tmp_path_factory.mktemp("slices")
    src, exe = str(d / "slices.cpp"), str(d / "slices")
    with open(src, "w") as f:
        f.write(PROGRAM % (sp.NTT_N_VEC, sp.NTT_LOG2, sp.FK20_N, sp.FK20_LOG2, sp.OPEN_N, sp.OPEN_LOG2, sp.HASH_N, sp.MAP_N, sp.VERIFY_N, sp.HASH_N, sp.HASH_N,
                           sp.HASH_N, sp.MAP_N, sp.MAP_N, sp.VERIFY_N, sp.VERIFY_N, sp.GROUPED_M, sp.COM_N))
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-3000:]
    return {k: (int(v[0]) if len(v) == 1 else tuple(int(x) for x in v)) for k, *v in (line.split() for line in out.stdout.split("\n") if line)}


@pytest.fixture(scope="module")
def calls():
    out = {}
    for flags in NTT_FLAGS:
        out["g1_ntt-flags%d" % flags] = sp.ntt_call(flags)
    out["g1_ntt-finite"] = sp.ntt_call(0, finite=True)
    for bitrev in (False, True):
        out["fk20-bitrev%d" % bitrev] = sp.fk20_call(bitrev)
        out["open-bitrev%d" % bitrev] = sp.open_call(bitrev)
    out["bls_field"], out["bls_hash"], out["bls_map"], out["bls_verify"] = sp.hash_call(False), sp.hash_call(True), sp.map_call(), sp.verify_call()
    return out


NAMES = ["g1_ntt-flags0", "g1_ntt-flags3", "g1_ntt-finite", "fk20-bitrev0", "fk20-bitrev1", "open-bitrev0", "open-bitrev1"]
BLS_NAMES = ["bls_field", "bls_hash", "bls_map", "bls_verify"]


# ------------------------------------------------------------------------------------------------------------------- slice sizes and shapes
def test_slice_lengths_are_the_headers_and_their_documented_formulas(header_slices):
    h = header_slices
    assert h["g1ntt"] == sp.NTT_SLICE == (1 << 18) // (1 << sp.NTT_LOG2) == 32768
    assert h["fk20"] == sp.FK20_SLICE == (1 << 17) // (1 << sp.FK20_LOG2) == 32768
    assert h["open"] == sp.OPEN_SLICE == (1 << 22) // (1 << sp.OPEN_LOG2) == 4096
    # at least one vector or polynomial where the floor would be zero or the quotient is small: N = 2^20, 2^19, 2^20
    assert (h["g1ntt_max"], h["fk20_max"], h["open_max"]) == (1, 1, 4)


def test_every_shape_crosses_its_boundaries_and_ends_in_a_short_slice(header_slices, calls):
    want = {"g1_ntt": (header_slices["g1ntt"], 3, 5), "fk20": (header_slices["fk20"], 2, 3), "open": (header_slices["open"], 2, 3)}
    for name in NAMES:
        c = calls[name]
        slice_len, n_slices, tail = want[name.split("-")[0]]
        assert c.slice == slice_len and len(c.starts) == n_slices and c.tail == tail and 0 < c.tail < c.slice, name
        assert c.starts == [s * slice_len for s in range(n_slices)] and c.n == (n_slices - 1) * slice_len + tail, name
        for arr, per in list(c.inputs.values()) + list(c.outputs.values()):
            assert arr.shape[0] == c.n * per and arr.flags.c_contiguous, name
    c = calls["g1_ntt-flags0"]
    assert c.n << sp.NTT_LOG2 == 524328 and (c.tail << sp.NTT_LOG2) // 2 == 20                   # points; butterflies of the last slice
    assert calls["fk20-bitrev0"].n << sp.FK20_LOG2 == 131084 and calls["open-bitrev0"].arg("evals").nbytes == 4099 << 15


def test_the_tail_is_unique_and_the_pool_size_divides_no_slice(calls):
    for name in NAMES:
        c = calls[name]
        tail = c.idx[c.n - c.tail:]
        assert len(set(tail.tolist())) == c.tail and not np.isin(c.idx[:c.n - c.tail], tail).any(), name
        n_pool = int(c.idx.max()) + 1
        assert n_pool in (11, 13) and c.slice % n_pool and set(c.idx.tolist()) == set(range(n_pool)), name
        # pseudo-random, not periodic: no shift by a slice, and no small shift, maps the sequence onto itself
        body = c.idx[:c.n - c.tail]
        for shift in list(range(1, 64)) + [c.slice]:
            if shift < len(body):
                assert (body[shift:] != body[:-shift]).mean() > 0.5, (name, shift)


# ------------------------------------------------------------------------------------------------------------------- identity entries and flags
def test_flags_are_set_on_both_sides_of_every_boundary(calls):
    for flags in NTT_FLAGS:
        c = calls["g1_ntt-flags%d" % flags]
        per = 1 << sp.NTT_LOG2
        for at in c.starts:
            w = sp.window(c, at)
            for name, (arr, _) in (("inf", c.inputs["inf"]), ("out_inf", c.outputs["out_inf"])):
                win = sp.rows(arr, per, at, w)
                assert win.any() and not win.all(), (flags, at, name)
            if at:
                assert sp.rows(c.arg("inf"), per, at - 64, 64).any() and sp.rows(c.want("out_inf"), per, at - 64, 64).any()
        assert {"holes", "identity"} <= set(c.pool["kinds"])
        # an identity entry is the point (0, 1) with its flag, never a stale finite point
        assert (c.arg("points")[c.arg("inf") == 1] == np.eye(1, 12, 6, dtype=np.uint64)[0]).all()
    c = calls["g1_ntt-finite"]
    assert not c.arg("inf").any() and c.want("out_inf").any()
    for bitrev in (False, True):
        c = calls["fk20-bitrev%d" % bitrev]
        per = 1 << sp.FK20_LOG2
        inf = c.want("inf").reshape(c.n, per)
        whole = inf.all(axis=1)                  # the zero and the constant polynomials
        assert whole[:c.slice].any() and whole[c.slice - 64:c.slice].any() and whole[c.slice:].any() and not whole[c.slice:].all()
        assert set(np.array(c.pool["kinds"])[np.unique(c.idx[whole])]) == {"zero", "constant"}


def test_in_domain_points_fall_in_both_slices_and_in_the_tail(calls):
    for bitrev in (False, True):
        c = calls["open-bitrev%d" % bitrev]
        inside = np.isin(c.iz, sp.IN_DOMAIN_Z)
        first, last = inside[:c.slice], inside[c.slice:]
        assert first[:64].any() and first[-64:].any() and last.any() and not last.all()
        for zid in sp.IN_DOMAIN_Z:                                                               # each of the three slots, many times
            assert (c.iz[:c.slice] == zid).sum() > 100
        assert (c.iz == 1).any() and sp.OPEN_Z_KINDS[1] == "zero"
        inf = c.want("inf")
        assert inf[:c.slice].any() and inf[c.slice:].any() and not inf[c.slice:].all()


# ------------------------------------------------------------------------------------------------------------------- no shift invariance
@pytest.mark.parametrize("name", NAMES + BLS_NAMES)
def test_no_slice_repeats_the_rows_of_another(calls, name):
    c = calls[name]
    arrays = list(c.inputs.items()) + list(c.outputs.items())
    for at in c.starts[1:]:
        w = sp.window(c, at)
        assert w == min(64, c.slice, c.n - at)
        for other in c.starts:
            if other == at:
                continue
            for what, (arr, per) in arrays:
                if name == "g1_ntt-finite" and what == "inf":
                    continue                                                                     # all zero: the call passes inf = NULL
                if what in getattr(c, "constant", ()):
                    continue                                                                     # hash_to_g2's flags: no message gives the identity
                assert sp.rows(arr, per, at, w).tobytes() != sp.rows(arr, per, other, w).tobytes(), (name, what, at, other)


# ------------------------------------------------------------------------------------------------------------------- mutations
@pytest.mark.parametrize("how", ["zero", "previous"])
@pytest.mark.parametrize("name", NAMES + BLS_NAMES)
def test_a_wrong_offset_in_any_slice_changes_every_output_array(calls, name, how):
    c = calls[name]
    assert set(c.outputs) == {"g1_ntt": {"out", "out_inf"}, "fk20": {"proof", "inf"}, "open": {"y", "proof", "inf"}, "bls_field": {"u"},
                              "bls_hash": {"points", "inf"}, "bls_map": {"points", "inf"}, "bls_verify": {"hq"}}[name.split("-")[0]]
    assert getattr(c, "constant", set()) == ({"inf"} if name == "bls_hash" else set())
    for what, (arr, per) in c.outputs.items():
        if what in getattr(c, "constant", ()):
            assert not arr.any()                 # zero in every slice under any reading: compared on the GPU, but it cannot tell offsets apart
            continue
        wrong = sp.reading(c, what, how)
        assert wrong.shape == arr.shape and wrong.tobytes() != arr.tobytes(), (name, what, how)
        # slice by slice: every slice after the first is wrong on its own, and the first is untouched
        assert sp.rows(wrong, per, 0, c.slice).tobytes() == sp.rows(arr, per, 0, c.slice).tobytes()
        for at in c.starts[1:]:
            cnt = min(c.slice, c.n - at)
            assert sp.rows(wrong, per, at, cnt).tobytes() != sp.rows(arr, per, at, cnt).tobytes(), (name, what, how, at)
            assert sp.first_difference(wrong, arr, per, c)["slice"] == 1
    if len(c.starts) > 2:                        # three slices: the two readings are different mistakes
        for what in c.outputs:
            assert sp.reading(c, what, "zero").tobytes() != sp.reading(c, what, "previous").tobytes(), (name, what)


# ------------------------------------------------------------------------------------------------------------------- hash-to-G2 and the BLS verifier
def test_bls_slice_lengths_shapes_and_tails(header_slices, calls):
    h = header_slices
    assert h["bls_const"] == h["bls_hash"] == h["bls_map"] == h["bls_verify"] == sp.BLS_SLICE == 1 << 17
    # a small call has the slice, and with it the stride of the point workspace, of its own size: 2 * 5 against 2 * 2^17 slots
    assert h["bls_small"] == 5 and h["bls_stride"] == 2 * sp.BLS_SLICE
    want = {"bls_field": (2, 61), "bls_hash": (2, 61), "bls_map": (3, 5), "bls_verify": (2, 6)}
    tails = {"bls_field": sp.HASH_TAIL, "bls_hash": sp.HASH_TAIL, "bls_map": sp.MAP_TAIL, "bls_verify": sp.VERIFY_TAIL}
    for name in BLS_NAMES:
        c = calls[name]
        n_slices, tail = want[name]
        assert c.slice == sp.BLS_SLICE and c.starts == [s * c.slice for s in range(n_slices)] and c.tail == tail == c.n - c.starts[-1], name
        for arr, per in list(c.inputs.values()) + list(c.outputs.values()):
            assert per == 1 and arr.shape[0] == c.n and arr.flags.c_contiguous, name
        # the last slice is made of pool items that occur nowhere before it, every one of them; the body uses all the others
        last, body = c.idx[c.n - c.tail:], c.idx[:c.n - c.tail]
        assert set(last.tolist()) == set(tails[name]) and set(body.tolist()) == set(range(sp.BLS_B)) - set(tails[name]), name
        assert sp.BLS_B == 13 and c.slice % sp.BLS_B
        for shift in list(range(1, 64)) + [c.slice]:
            if shift < len(body):
                assert (body[shift:] != body[:-shift]).mean() > 0.5, (name, shift)
    assert calls["bls_map"].tail == len(sp.MAP_TAIL) and calls["bls_verify"].tail == len(sp.VERIFY_TAIL)          # distinct items
    # 61 messages: 122 lanes of k_h2c_clear, one full wavefront and a partial one
    assert 2 * calls["bls_hash"].tail == 64 + 58


def test_bls_messages_are_packed_as_the_pool_has_them(calls):
    for name in ("bls_field", "bls_hash", "bls_verify"):
        c = calls[name]
        off, msgs = c.offsets, c.pool["msgs"]
        base = sp.VERIFY_BASE if name == "bls_verify" else sp.HASH_BASE
        assert off.dtype == np.uint64 and off.shape == (c.n + 1,) and int(off[0]) == base > 0 and int(off[-1]) == c.msgs.size
        assert (c.msgs[:base] == 0xA5).all() and (np.diff(off.astype(np.int64)) == np.array([len(x) for x in msgs])[c.idx]).all()
        for j in (0, 1, 2, c.slice - 1, c.slice, c.slice + 1, c.n - 2, c.n - 1):
            assert c.msgs[int(off[j]):int(off[j + 1])].tobytes() == msgs[c.idx[j]], (name, j)
        lens = np.diff(off.astype(np.int64))
        for at in c.starts:                                                                      # mixed lengths inside every wavefront's reach
            assert len(set(lens[at:at + sp.window(c, at)].tolist())) >= 4, (name, at)
    c = calls["bls_hash"]
    assert tuple(len(x) for x in c.pool["msgs"]) == sp.HASH_LENGTHS and {0, 1, 55, 56, 64, 119, 120} <= set(sp.HASH_LENGTHS)
    assert (np.diff(c.offsets.astype(np.int64))[:c.slice] == 0).any()                            # the empty message


def test_bls_identity_outputs_on_both_sides_of_every_boundary(calls):
    c = calls["bls_map"]
    inf = c.want("inf")
    assert inf[c.n - c.tail:].tolist() == [int(j == sp.MAP_INF) for j in sp.MAP_TAIL] and inf[c.n - c.tail:].sum() == 1
    for at in c.starts[:-1]:
        assert inf[at:at + 64].any() and not inf[at:at + 64].all() and inf[at + c.slice - 64:at + c.slice].any()
    assert (c.want("points")[inf == 1] == np.eye(1, 24, 12, dtype=np.uint64)[0]).all()


def test_bls_pools_are_consistent_by_a_second_route(calls):
    import bls12_381_model as m
    import bls_replay_cases as brc
    import h2c_model as h
    p = sp.hash_pool()
    for j, msg in enumerate(p["msgs"]):
        u0, u1 = h.hash_to_field_g2(msg, brc.DST)
        assert _ints(p["u"][j].reshape(4, 6)) == [u0[0], u0[1], u1[0], u1[1]]
        q = m.g2_add(h.iso3(h.sswu(u0)[0]), h.iso3(h.sswu(u1)[0]))
        assert p["pts"][j] == h.clear_cofactor_h_eff(q) and p["pts"][j] is not None           # the psi formula made it; [h_eff] is the other route
        assert h.words_g2(p["points"][j], p["inf"][j]) == p["pts"][j]
    p = sp.map_pool()
    assert [q is None for q in p["pts"]] == [j in (sp.MAP_INF, sp.MAP_INF_BODY) for j in range(sp.BLS_B)]
    for (u0, u1), q, row, flag in zip(p["us"], p["pts"], p["points"], p["inf"]):
        assert q == h.clear_cofactor_h_eff(m.g2_add(h.iso3(h.sswu(u0)[0]), h.iso3(h.sswu(u1)[0]))) and h.words_g2(row, flag) == q
    p = sp.verify_pool()
    assert len(p["pool"]) == sp.BLS_B
    for j, (sk, pk, msg, sig) in enumerate(p["pool"]):
        assert h.verify(pk, msg, sig, brc.DST) and pk == h.sk_to_pk(sk)
        assert h.words_g2(p["hq"][j], 0) == brc.hashed(msg, brc.DST) and h.words_g2(p["sig"][j], 0) == sig
    c = calls["bls_verify"]
    assert c.forged == (c.slice - 1, c.slice, c.n - 1)
    for j in c.forged:                                                                           # the forgeries of test_gpu_slices.py are forgeries
        sk, pk, msg, sig = p["pool"][c.idx[j]]
        bad = sp.forged_messages(c, j)
        assert len(msg) > 0 and (bad != c.msgs).sum() == 1
        lst = sp.message_list(c, bad)
        assert lst[j] != msg and len(lst[j]) == len(msg) and lst[j - 1] == p["msgs"][c.idx[j - 1]]
        assert not h.verify(pk, lst[j], sig, brc.DST)
    assert sp.message_list(c)[c.slice] == p["msgs"][c.idx[c.slice]] and (c.arg("rand") != 0).all()


# ------------------------------------------------------------------------------------------------------------------- the pools on integers
def _ints(rows):
    return [int.from_bytes(r.tobytes(), "little") for r in rows]


def test_g1_ntt_pool_the_inverse_transform_gives_the_vector_back():
    for flags, finite in ((0, False), (pm.INVERSE | pm.BITREV, False), (0, True)):
        p = sp.ntt_pool(flags, finite)
        assert len(p["vecs"]) == sp.NTT_B == 13
        for v, out in zip(p["vecs"], p["outs"]):
            assert pm.ntt_flags(out, sp.NTT_LOG2, flags ^ pm.INVERSE) == v and len(out) == 8
        if not (flags & pm.INVERSE):
            assert p["outs"][0] == pm.ntt_definition(p["vecs"][0], sp.NTT_LOG2, bitrev=bool(flags & pm.BITREV))
        assert p["inf"].tolist() == [int(e == 0) for v in p["vecs"] for e in v]
        assert p["out_inf"].tolist() == [int(e == 0) for v in p["outs"] for e in v]


def test_fk20_pool_the_circulant_pipeline_equals_the_quotient_formula(calls):
    for bitrev in (False, True):
        p = sp.fk20_pool(bitrev)
        assert len(p["polys"]) == sp.FK20_B == 11
        for f, e in zip(p["polys"], p["exps"]):
            assert fm.fk20_proofs(f, sp.TAU, sp.FK20_LOG2, bitrev) == e
        c = calls["fk20-bitrev%d" % bitrev]
        for j in (0, 1, c.slice - 1, c.slice, c.n - 1):                                            # the assembled rows are the pool's integers
            assert _ints(sp.rows(c.arg("coeffs"), 4, j, 1)) == p["polys"][c.idx[j]]
            assert sp.rows(c.want("inf"), 4, j, 1).tolist() == [int(e == 0) for e in p["exps"][c.idx[j]]]


def test_opening_pool_y_is_horner_and_in_the_domain_the_evaluation_of_the_slot(calls):
    for bitrev in (False, True):
        p = sp.open_pool(bitrev)
        st = p["setup"]
        assert sum(st.lagrange_tau) % R == 1 and st.n == 1024 and sp.OPEN_POLY_KINDS.count("random") == 10
        slot_of = {"slot0": 0, "slot1": 1, "slotlast": st.n - 1}
        for b in range(sp.OPEN_B):
            # a commitment in the slot order of the evaluations: sum f(slot_i) l_i(tau) = f(tau)
            assert sum(e * l for e, l in zip(p["evals_int"][b], st.lagrange_tau)) % R == p["f_tau"][b]
            for zid in sp.IN_DOMAIN_Z:
                m = slot_of[sp.OPEN_Z_KINDS[zid]]
                assert p["zs"][zid] == st.slot_domain[m] and p["y_int"][b][zid] == p["evals_int"][b][m]
            for zid in range(sp.OPEN_C):
                assert (p["q"][b][zid] * (sp.TAU - p["zs"][zid]) + p["y_int"][b][zid]) % R == p["f_tau"][b]
        c = calls["open-bitrev%d" % bitrev]
        for j in (0, 1, c.slice - 1, c.slice, c.slice + 1, c.n - 1):
            f, zed = p["polys"][c.idx[j]], _ints(c.arg("z")[j:j + 1])[0]
            assert zed == p["zs"][c.iz[j]] and _ints(c.want("y")[j:j + 1])[0] == prc.horner(f, zed)
            ev = _ints(sp.rows(c.arg("evals"), st.n, j, 1))
            assert ev == p["evals_int"][c.idx[j]] and ev[5] == prc.horner(f, st.slot_domain[5])
        assert c.want("inf")[c.n - 3:].tolist() == [0, 1, 0] and sp.OPEN_POLY_KINDS[sp.OPEN_TAIL[1]] == "constant"


# ------------------------------------------------------------------------------------------------------------------- min-sig, grouped and committees
# The same conditions for the sliced calls of csrc/zkp_bls_minsig.hip (MINSIG_NAMES) and for the two verifiers that drive sliced callees on
# m messages or n committees (DRIVER_NAMES): slice lengths from the planning headers, shapes and tails, no shift invariance, the two wrong
# readings, the packing, and the pools by a second route.
MINSIG_NAMES = ["minsig_field", "minsig_map", "minsig_clear", "minsig_verify", "minsig_samekey"]
DRIVER_NAMES = ["grouped", "committees"]
OUTPUTS = {"minsig_field": {"u"}, "minsig_map": {"points", "inf"}, "minsig_clear": {"points", "inf"}, "minsig_verify": {"hp"}, "minsig_samekey": {"hp"},
           "grouped": {"hq"}, "committees": {"apk", "hq"}}


@pytest.fixture(scope="module")
def more_calls():
    return {"minsig_field": sp.minsig_field_call(), "minsig_map": sp.minsig_map_call(), "minsig_clear": sp.minsig_clear_call(),
            "minsig_verify": sp.minsig_verify_call(False), "minsig_samekey": sp.minsig_verify_call(True), "grouped": sp.grouped_call(),
            "committees": sp.committees_call()}


def test_minsig_slice_lengths_shapes_and_tails(header_slices, more_calls):
    h = header_slices
    for k in ("minsig_const", "minsig_field", "minsig_map", "minsig_clear", "minsig_verify", "minsig_samekey", "bls_grouped", "bls_committees"):
        assert h[k] == sp.BLS_SLICE == 1 << 17, k
    assert h["minsig_small"] == (5, 5, 5)                                                         # a call of 5 has the slice, and the strides, of its own size
    want = {"minsig_field": (2, 61), "minsig_map": (3, 5), "minsig_clear": (3, 5), "minsig_verify": (2, 6), "minsig_samekey": (2, 6), "grouped": (2, 6),
            "committees": (2, 6)}
    tails = {"minsig_field": sp.HASH_TAIL, "minsig_map": sp.MAP_TAIL, "minsig_clear": sp.MAP_TAIL}
    for name in MINSIG_NAMES + DRIVER_NAMES:
        c = more_calls[name]
        n_slices, tail = want[name]
        ids = tails.get(name, sp.VERIFY_TAIL)
        assert c.slice == sp.BLS_SLICE and c.starts == [s * c.slice for s in range(n_slices)] and c.tail == tail == c.n - c.starts[-1], name
        assert set(c.outputs) == OUTPUTS[name] and c.constant == set(), name
        for arr, per in list(c.inputs.values()) + list(c.outputs.values()):
            assert per == 1 and arr.shape[0] == c.n and arr.flags.c_contiguous, name
        last, body = c.idx[c.n - c.tail:], c.idx[:c.n - c.tail]
        assert set(last.tolist()) == set(ids) and set(body.tolist()) == set(range(sp.BLS_B)) - set(ids), name
        assert name == "minsig_field" or last.tolist() == list(ids), name                         # distinct items
        assert sp.BLS_B == 13 and c.slice % sp.BLS_B
        for shift in list(range(1, 64)) + [c.slice]:
            if shift < len(body):
                assert (body[shift:] != body[:-shift]).mean() > 0.5, (name, shift)
    assert 2 * more_calls["minsig_field"].tail == 64 + 58                                         # k_g1h_map: one full wavefront and a partial one
    assert more_calls["minsig_field"].tail == 61 and more_calls["minsig_map"].tail == 5           # k_g1h_clear / k_g1h_affine: partial wavefronts


@pytest.mark.parametrize("name", MINSIG_NAMES + DRIVER_NAMES)
def test_minsig_no_slice_repeats_the_rows_of_another(more_calls, name):
    c = more_calls[name]
    arrays = list(c.inputs.items()) + list(c.outputs.items())
    assert len(arrays) >= 2
    for at in c.starts[1:]:
        w = sp.window(c, at)
        assert w == min(64, c.slice, c.n - at)
        for other in c.starts:
            if other == at:
                continue
            for what, (arr, per) in arrays:
                assert sp.rows(arr, per, at, w).tobytes() != sp.rows(arr, per, other, w).tobytes(), (name, what, at, other)


@pytest.mark.parametrize("how", ["zero", "previous"])
@pytest.mark.parametrize("name", MINSIG_NAMES + DRIVER_NAMES)
def test_minsig_a_wrong_offset_in_any_slice_changes_every_output_array(more_calls, name, how):
    c = more_calls[name]
    assert set(c.outputs) == OUTPUTS[name] and c.constant == set()                                # no constant output: every array tells offsets apart
    for what, (arr, per) in c.outputs.items():
        wrong = sp.reading(c, what, how)
        assert wrong.shape == arr.shape and wrong.tobytes() != arr.tobytes(), (name, what, how)
        assert sp.rows(wrong, per, 0, c.slice).tobytes() == sp.rows(arr, per, 0, c.slice).tobytes()
        for at in c.starts[1:]:
            cnt = min(c.slice, c.n - at)
            assert sp.rows(wrong, per, at, cnt).tobytes() != sp.rows(arr, per, at, cnt).tobytes(), (name, what, how, at)
            assert sp.first_difference(wrong, arr, per, c)["slice"] == 1
    if len(c.starts) > 2:
        for what in c.outputs:
            assert sp.reading(c, what, "zero").tobytes() != sp.reading(c, what, "previous").tobytes(), (name, what)


def test_minsig_messages_are_packed_as_the_pool_has_them(more_calls):
    for name in ("minsig_field", "minsig_verify", "minsig_samekey", "grouped", "committees"):
        c = more_calls[name]
        off, msgs = c.offsets, c.pool["msgs"]
        base = sp.HASH_BASE if name == "minsig_field" else sp.VERIFY_BASE
        assert off.dtype == np.uint64 and off.shape == (c.n + 1,) and int(off[0]) == base > 0 and int(off[-1]) == c.msgs.size
        assert (c.msgs[:base] == 0xA5).all() and (np.diff(off.astype(np.int64)) == np.array([len(x) for x in msgs])[c.idx]).all()
        for j in (0, 1, 2, c.slice - 1, c.slice, c.slice + 1, c.n - 2, c.n - 1):
            assert c.msgs[int(off[j]):int(off[j + 1])].tobytes() == msgs[c.idx[j]], (name, j)
        lens = np.diff(off.astype(np.int64))
        for at in c.starts:
            assert len(set(lens[at:at + sp.window(c, at)].tolist())) >= 4, (name, at)
    c = more_calls["minsig_field"]
    assert tuple(len(x) for x in c.pool["msgs"]) == sp.HASH_LENGTHS and (np.diff(c.offsets.astype(np.int64))[:c.slice] == 0).any()


def test_minsig_identity_outputs_on_both_sides_of_every_boundary(more_calls):
    for name in ("minsig_map", "minsig_clear"):
        c = more_calls[name]
        inf = c.want("inf")
        assert inf[c.n - c.tail:].sum() == 1 and inf[c.n - c.tail:].tolist() == [int(j == sp.MAP_INF) for j in sp.MAP_TAIL], name
        for at in c.starts[:-1]:
            assert inf[at:at + 64].any() and not inf[at:at + 64].all() and inf[at + c.slice - 64:at + c.slice].any(), (name, at)
        assert (c.want("points")[inf == 1] == np.eye(1, 12, 6, dtype=np.uint64)[0]).all()
    c = more_calls["minsig_clear"]
    assert sp.CLEAR_FLAGGED_TAIL == sp.MAP_INF and {"identity", "order3_plus", "order11"} <= set(c.pool["names"])
    fin = c.arg("inf")                                                                            # the input flags: one flagged item in the body, one in the tail
    assert fin[c.n - c.tail:].sum() == 1 and all(fin[at:at + c.slice].any() for at in c.starts[:-1])
    names = np.array(c.pool["names"])
    for at in c.starts[:-1]:                                                                      # every kind of identity in every full slice, unflagged ones among them
        assert {"identity", "order3_plus", "order3_minus", "order11"} <= set(names[c.idx[at:at + c.slice]])
    assert ((c.want("inf") == 1) & (fin == 0)).any() and c.want("inf").sum() > 2 * fin.sum()


def test_minsig_pools_are_consistent_by_a_second_route(more_calls):
    import h2c_model as h
    import h2g1_model as g
    import minsig_replay_cases as mrc
    p = sp.minsig_field_pool()
    for j, msg in enumerate(p["msgs"]):
        assert _ints(p["u"][j].reshape(2, 6)) == list(g.hash_to_field_g1(msg, mrc.DST))
    p = sp.minsig_map_pool()
    assert [q is None for q in p["pts"]] == [j in (sp.MAP_INF, sp.MAP_INF_BODY) for j in range(sp.BLS_B)]
    for (u0, u1), q, row, flag in zip(p["us"], p["pts"], p["points"], p["inf"]):
        assert q == g.clear_cofactor(g.e_add(g.iso11(g.sswu(u0)[0]), g.iso11(g.sswu(u1)[0]))) and g.words_g1(row, flag) == q
        assert g.in_g1(q)
    p = sp.minsig_clear_pool()
    assert p["pts_inf"].tolist() == [int(q is None) for q in p["pts"]] and p["pts"][0] == (0, 2)
    for q, out, row, flag in zip(p["pts"], p["outs"], p["points"], p["inf"]):
        assert g.e_on_curve(q) and g.words_g1(row, flag) == out and g.in_g1(out)
        assert out == g.e_add(q, g.e_mul(q, g.X_ABS))                                             # [1 - x] P = P + [|x|] P: x is negative
    assert [o is None for o in p["outs"]] == [k in ("order3_plus", "order3_minus", "identity", "order11", "flagged_generator") for k in p["names"]]
    for same_key in (False, True):
        name = "minsig_samekey" if same_key else "minsig_verify"
        c = more_calls[name]
        p = c.pool
        assert len(p["pool"]) == sp.BLS_B and len({x[0] for x in p["pool"]}) == (1 if same_key else sp.BLS_B)
        for j, (sk, pk, msg, sig) in enumerate(p["pool"]):
            hp = mrc.hashed(msg, mrc.DST)
            u0, u1 = g.hash_to_field_g1(msg, mrc.DST)
            assert hp == g.clear_cofactor(g.e_add(g.iso11(g.sswu(u0)[0]), g.iso11(g.sswu(u1)[0])))
            assert g.words_g1(p["hp"][j], 0) == hp and g.words_g1(p["sig"][j], 0) == sig and h.words_g2(p["pk"][j], 0) == pk == g.sk_to_pk(sk)
            assert g.in_g1(sig) and sig == g.e_mul(hp, sk) and g.verify(pk, msg, sig, mrc.DST)
        assert c.forged == (c.slice - 1, c.slice, c.n - 1) and (c.arg("rand") != 0).all()
        for j in c.forged:
            sk, pk, msg, sig = p["pool"][c.idx[j]]
            bad = sp.forged_messages(c, j)
            lst = sp.message_list(c, bad)
            assert len(msg) > 0 and (bad != c.msgs).sum() == 1 and lst[j] != msg and len(lst[j]) == len(msg) and lst[j - 1] == p["msgs"][c.idx[j - 1]]
            assert g.hash_to_g1(lst[j], mrc.DST) != mrc.hashed(msg, mrc.DST)                      # another point: [sk] of it is another signature
        sig, moved = sp.shifted_signature(c, c.shifted)
        assert c.shifted == c.slice + 2 and g.e_on_curve(moved) and not g.in_g1(moved) and (sig != c.arg("sig")).any(axis=1).sum() == 1
        assert g.e_mul(moved, 3) == g.e_mul(p["pool"][c.idx[c.shifted]][3], 3)
    assert more_calls["minsig_samekey"].pk1.shape == (1, 24) and more_calls["minsig_verify"].flagged_pk == sp.BLS_SLICE + 1


def test_grouped_and_committee_calls_are_what_their_pools_sign(more_calls):
    import agg_model as am
    import bls_replay_cases as brc
    import bls12_381_model as m
    import h2c_model as h
    from h2g1_model import words_g1
    c = more_calls["grouped"]
    p = c.pool
    m_msgs, n = c.n, c.member.size
    assert n == m_msgs + 1 == int(c.grp_off[-1]) and c.grp_off.dtype == np.uint64 and int(c.grp_off[0]) == 0
    assert {g: int(c.sizes[g]) for g in sp.GROUPED_SIZES} == {5: 0, 6: 2, c.slice - 2: 0, c.slice: 3} and (np.delete(c.sizes, list(sp.GROUPED_SIZES)) == 1).all()
    assert (np.diff(c.grp_off.astype(np.int64)) == c.sizes).all() and c.pk.shape == (n, 12) and c.sig.shape == (n, 24) and c.rand.shape == (n, 2)
    for i in (0, 5, 6, 7, n // 2, n - 1):                                                         # signature i is its group's pool item
        g = int(c.member[i])
        assert int(c.grp_off[g]) <= i < int(c.grp_off[g + 1]) and c.pk[i].tobytes() == p["pk"][c.idx[g]].tobytes() and c.sig[i].tobytes() == p["sig"][c.idx[g]].tobytes()
    assert (c.rand != 0).all() and len({tuple(r) for r in c.rand[int(c.grp_off[c.slice]):int(c.grp_off[c.slice + 1])].tolist()}) == 3
    for j in c.forged:                                                                            # a changed message matters only where somebody signed it
        sk, pk, msg, sig = p["pool"][c.idx[j]]
        lst = sp.message_list(c, sp.forged_messages(c, j))
        assert c.sizes[j] >= 1 and len(msg) > 0 and lst[j] != msg and not h.verify(pk, lst[j], sig, brc.DST)
    assert c.forged == (c.slice - 1, c.slice + 1, m_msgs - 1) and c.moved == c.slice + 1
    assert c.idx[c.moved] != c.idx[c.moved - 1] and c.sizes[c.moved] == 1                         # the moved signature lands under another message
    sk, pk, msg, sig = p["pool"][c.idx[c.moved]]
    assert not h.verify(pk, p["msgs"][c.idx[c.moved - 1]], sig, brc.DST)
    buf, off = sp.expanded_messages(c)
    assert off.shape == (n + 1,) and int(off[0]) == sp.VERIFY_BASE
    for i in (0, 6, 7, n - 1):
        assert buf[int(off[i]):int(off[i + 1])].tobytes() == p["msgs"][c.idx[c.member[i]]]
    c = more_calls["committees"]
    p = c.pool
    sks, pks = am.key_table(sp.COM_TABLE)
    assert tuple(len(e) for e in p["entries"]) == sp.COM_SIZES and sorted(set(sp.COM_SIZES)) == [1, 2, 3, 4, 5, 7, 33]
    assert any(e & am.SIGN for x in p["entries"] for e in x) and all(not x[0] & am.SIGN for x in p["entries"])
    sizes = np.diff(c.seg_off.astype(np.int64))
    assert (sizes == np.array(sp.COM_SIZES)[c.idx]).all() and c.entries.size == int(c.seg_off[-1]) < 8 * c.n and c.entries.dtype == np.uint32
    assert (sizes[:c.slice] == 33).sum() > 1000 and sp.COM_SIZES[6] == 33 and 6 not in sp.VERIFY_TAIL
    for j in (0, 1, c.slice - 1, c.slice, c.n - 1):
        assert c.entries[int(c.seg_off[j]):int(c.seg_off[j + 1])].tolist() == p["entries"][c.idx[j]]
    for j, (e, sk, msg) in enumerate(zip(p["entries"], p["sks"], p["msgs"])):
        acc = None
        for x in e:
            acc = m.g1_add(acc, m.g1_neg(pks[x & am.ROW]) if x & am.SIGN else pks[x & am.ROW])
        assert acc == am.public_key(sk) and words_g1(p["apk"][j], 0) == acc                       # the signed sum of the keys is the key of the signed sum
        assert h.verify(acc, msg, h.words_g2(p["sig"][j], 0), brc.DST) and h.words_g2(p["hq"][j], 0) == brc.hashed(msg, brc.DST)
    for j in c.forged:                                                                            # another member: another aggregate key under the same signature
        entries, other = sp.swapped_member(c, j)
        e = p["entries"][c.idx[j]]
        assert other not in {x & am.ROW for x in e} and (entries != c.entries).sum() == 1
        assert (p["sks"][c.idx[j]] - sks[e[0]] + sks[other]) % h.R_ORDER != p["sks"][c.idx[j]]
    assert c.forged == (c.slice - 1, c.slice, c.n - 1)
