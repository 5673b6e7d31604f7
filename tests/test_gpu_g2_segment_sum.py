"""zkp_g2_segment_sum_batch on one MI355X through the C ABI (run with -m gpu).  Every case sums rows of ONE table of 37 model points of
G2 (36 points and their total, tests/agg_g2_model.py) and compares out, out_inf and status byte for byte with the model's sums, in the
host flavour and in the _dev flavour.  The shapes are those of tests/test_gpu_segment_sum.py: the smallest that reach each path of the
run-wise sum (runs of 32 entries, two partials per run and level) and of the shared inversion (wavefronts of 64 sums: k_agg2_affine has
one lane per sum).  One-entry segments leave their row as the sum with Z = 1, whose second coefficient is zero."""
import ctypes
import random

import numpy as np
import pytest

import agg_g2_model as a2
import agg_model as am
import bls12_381_model as m
import h2c_model as h
import outside_groups as og
from test_gpu_segment_sum import MALFORMED, _dev, _off

pytestmark = pytest.mark.gpu
N_KEYS = 36
TOTAL = 36          # the row that holds the sum of the 36 points
N_TABLE = 37
IDENTITY = [0] * 12 + [1] + [0] * 11


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def table():
    """(model points, rows (37, 24))"""
    pts = list(a2.g2_table(N_KEYS))
    pts.append(a2.g2_sum(pts))
    return pts, a2.g2_rows(pts)[0]


def run_dev(eng, rows, idx, seg_off, n_table=N_TABLE):
    """the _dev flavour on resident tensors: (out, inf, status) as numpy"""
    import torch
    a_idx, a_off = am.entry_arrays(idx, seg_off)
    out, inf, st = eng.g2_segment_sum(_dev(rows[:n_table]), _dev(a_idx), _dev(a_off))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), inf.cpu().numpy(), st.cpu().numpy()


def check(eng, table, idx, seg_off, host=True):
    pts, rows = table
    want = a2.sum_rows(pts, idx, seg_off)
    got = run_dev(eng, rows, idx, seg_off, n_table=len(pts))
    for g, w, what in zip(got, want, ("out", "out_inf", "status")):
        assert g.tobytes() == w.tobytes(), "_dev flavour: %s differs" % what
    if host:
        a_idx, a_off = am.entry_arrays(idx, seg_off)
        got = eng.g2_segment_sum(rows, a_idx, a_off)
        for g, w, what in zip(got, want, ("out", "out_inf", "status")):
            assert g.tobytes() == w.tobytes(), "host flavour: %s differs" % what
    return want


def _rows(n, seed, signs=True):
    rng = random.Random(seed)
    return [rng.randrange(N_KEYS) | (am.SIGN if signs and rng.randrange(4) == 0 else 0) for _ in range(n)]


def test_run_borders_inside_at_and_across_segments_and_empty_segments(eng, table):
    lens = (1, 31, 1, 32, 33, 0, 64, 0, 0, 2)
    _, inf, st = check(eng, table, _rows(sum(lens), 1), _off(lens))
    assert inf.tolist() == [0, 0, 0, 0, 0, 1, 0, 1, 1, 0] and not st.any()


@pytest.mark.parametrize("long", [513, 8193])
def test_a_long_segment_beside_one_entry_neighbours_takes_three_and_four_levels(eng, table, long):
    """513 entries leave 34 partials and then 4: three levels; 8193 leave 514, 34, 4: four"""
    lens = (1, long, 1)
    _, inf, st = check(eng, table, _rows(sum(lens), long), _off(lens))
    assert not inf.any() and not st.any()


def test_one_entry_segments_that_share_a_run(eng, table):
    idx = _rows(33, 33, signs=False)
    want, _, _ = check(eng, table, idx, _off((1,) * 33))
    assert want.tobytes() == table[1][idx].tobytes()


@pytest.mark.parametrize("n_seg", [1, 63, 64, 65, 130])
def test_identities_at_the_borders_of_the_shared_inversion(eng, table, n_seg):
    """identities (an empty segment, a cancelling pair) at the first and the last lane of a wavefront, and at 130 sums the whole second
    wavefront: a zero norm that entered the shared product would zero every sum of its wavefront"""
    rng = random.Random(n_seg)
    dead = {0, n_seg - 1, 63} if n_seg > 1 else set()
    if n_seg == 130:
        dead |= set(range(64, 128))
    idx, lens = [], []
    for j in range(n_seg):
        if j in dead and j % 2:
            r = rng.randrange(N_KEYS)
            seg = [r, r | am.SIGN]                    # a + (-a)
        elif j in dead:
            seg = []
        else:
            seg = [rng.randrange(N_KEYS) for _ in range(1 + j % 3)]
        idx += seg
        lens.append(len(seg))
    _, inf, st = check(eng, table, idx, _off(lens))
    assert [j for j in range(n_seg) if inf[j]] == sorted(j for j in dead if j < n_seg) and not st.any()
    if n_seg == 1:
        _, inf, _ = check(eng, table, [], [0, 0])     # the one sum is the identity
        assert inf.tolist() == [1]


def test_one_row_forty_times_is_a_doubling_and_then_a_chain(eng, table):
    pts, _ = table
    want, _, _ = check(eng, table, [5] * 40 + [7], _off((40, 1)))
    assert want[0].tolist() == a2.g2_rows([m.g2_mul(pts[5], 40)])[0][0].tolist()
    want, _, _ = check(eng, table, [5 | am.SIGN] * 40, _off((40,)))
    assert want[0].tolist() == a2.g2_rows([m.g2_neg(m.g2_mul(pts[5], 40))])[0][0].tolist()


def test_a_row_and_its_negative_cancel(eng, table):
    a, b = 3, 11
    idx = [a, a | am.SIGN, a, a | am.SIGN, b, a, b, a | am.SIGN, b | am.SIGN, a | am.SIGN, a]
    want, inf, _ = check(eng, table, idx, _off((2, 3, 4, 2)))
    assert inf.tolist() == [1, 0, 1, 1] and want[1].tobytes() == table[1][b].tobytes()


def test_the_total_minus_the_absent_is_the_sum_of_the_rest(eng, table):
    import zkvm_pairings_amd as z
    pts, rows = table
    x, y = 4, 29
    rest = a2.g2_sum(pts[r] for r in range(N_KEYS) if r not in (x, y))
    idx, seg_off = z.committee_entries([[x, y], []], absent_from=TOTAL)
    assert idx.tolist() == [TOTAL, x | am.SIGN, y | am.SIGN, TOTAL]
    want, _, _ = check(eng, table, idx.tolist(), seg_off.tolist())
    assert want[0].tobytes() == a2.g2_rows([rest])[0][0].tobytes() and want[1].tobytes() == rows[TOTAL].tobytes()
    for helper in (z.bls_minsig_aggregate_keys, z.bls_aggregate_signatures):
        got, inf = helper(rows, [[x, y], []], absent_from=TOTAL, engine=eng)
        assert got.tobytes() == want.tobytes() and not inf.any()
        every = helper(rows, [list(range(N_KEYS))], engine=eng)[0]
        assert every[0].tobytes() == rows[TOTAL].tobytes()
    bits = [[1 if r not in (x, y) else 0 for r in range(N_KEYS)]]
    got, _ = z.bls_aggregate_signatures(rows, [list(range(N_KEYS))], bits=bits, engine=eng)
    assert got[0].tobytes() == want[0].tobytes()


@pytest.mark.parametrize("row", [N_TABLE, 0x7FFFFFFF, N_TABLE | am.SIGN])
def test_a_row_beyond_the_table_refuses_its_segment_and_leaves_the_neighbours(eng, table, row):
    lens = (3, 40, 2)
    idx = _rows(sum(lens), 7)
    idx[3 + 17] = row
    want, inf, st = check(eng, table, idx, _off(lens), host=False)
    assert st.tolist() == [0, 1, 0] and inf.tolist() == [0, 1, 0] and want[1].tolist() == IDENTITY


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_offsets_refuse_every_segment_and_raise_the_validation_word(kind):
    from zkvm_pairings_amd import PairingEngine
    rows = a2.g2_rows(a2.g2_table(N_KEYS))[0]
    idx, off = _rows(45, 2), MALFORMED[kind]
    e = PairingEngine(0, validate=True)
    try:
        out, inf, st = run_dev(e, rows, idx, off, n_table=N_KEYS)
        assert st.tolist() == [1, 1, 1] and inf.tolist() == [1, 1, 1] and out.tobytes() == a2.g2_rows([None] * 3)[0].tobytes()
        assert e.take_validation_status() is True
        out, inf, st = run_dev(e, rows, idx, [0, 5, 9, 45], n_table=N_KEYS)          # the next call is not tainted
        assert not st.any() and not inf.any() and e.take_validation_status() is False
    finally:
        e.close()
    e = PairingEngine(0)
    try:
        _, inf, st = run_dev(e, rows, idx, off, n_table=N_KEYS)                      # without validation mode: the same sums, no word
        assert st.tolist() == [1, 1, 1] and inf.tolist() == [1, 1, 1] and e.take_validation_status() is False
    finally:
        e.close()


def test_the_host_flavour_refuses_what_it_can_see(eng, table):
    _, rows = table
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    out, inf, st = np.full((3, 24), 7, dtype=np.uint64), np.full(3, 7, dtype=np.uint8), np.full(3, 7, dtype=np.uint8)

    def call(n_table, idx, off):
        a_idx, a_off = am.entry_arrays(idx, off)
        return eng._lib.zkp_g2_segment_sum_batch(eng._h, p(rows), n_table, p(a_idx) if a_idx.size else None, a_idx.size, p(a_off), len(off) - 1, p(out), p(inf),
                                                 p(st))
    idx = _rows(45, 2)
    for off in MALFORMED.values():
        assert call(N_TABLE, idx, off) == -1
    bad = list(idx)
    bad[44] = N_TABLE
    assert call(N_TABLE, bad, [0, 5, 9, 45]) == -1
    assert call(0, idx, [0, 5, 9, 45]) == -1                                        # entries and no table
    assert call((1 << 24) + 1, idx, [0, 5, 9, 45]) == -1
    assert eng._lib.zkp_g2_segment_sum_batch(eng._h, p(rows), N_TABLE, None, 45, p(out), 3, p(out), p(inf), p(st)) == -1
    assert (out == 7).all() and (inf == 7).all() and (st == 7).all()
    assert call(N_TABLE, idx, [0, 5, 9, 45]) == 0 and not st.any()
    assert call(0, [], [0, 0, 0, 0]) == 0 and inf.tolist() == [1, 1, 1]               # no table, no entries: three identities


def test_a_row_on_the_twist_outside_g2_is_summed_like_any_other(eng, table):
    """the table is the caller's to validate: a point of the curve outside the subgroup goes through the curve's law, alone (Z = 1), doubled,
    added to points of G2 and cancelled"""
    pts, _ = table
    outside = [q for q in og.g2_points().values() if q is not None and m.g2_on_curve(q) and not m.g2_torsion_free(q)]
    assert outside
    mixed = list(pts[:5]) + [outside[0]]
    tab = (mixed, a2.g2_rows(mixed)[0])
    idx = [5, 5, 5, 0, 5, 1, 2, 5 | am.SIGN, 5, 5 | am.SIGN, 3]
    want, inf, st = check(eng, tab, idx, _off((1, 2, 5, 2, 1)))
    assert inf.tolist() == [0, 0, 0, 1, 0] and not st.any()
    assert want[0].tobytes() == tab[1][5].tobytes() and not m.g2_torsion_free(h.words_g2(want[1].tolist(), 0))
