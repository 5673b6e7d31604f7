"""zkp_g1_segment_sum_batch on one MI355X through the C ABI (run with -m gpu).  Every case sums rows of ONE table of 37 model points
(36 keys and their total, tests/agg_model.py) and compares out, out_inf and status byte for byte with the model's sums, in the host
flavour and in the _dev flavour.  The shapes are the smallest that reach each path of the run-wise sum (runs of 32 entries, two partials
per run and level) and of the shared inversion (wavefronts of 64 sums)."""
import ctypes
import random

import numpy as np
import pytest

import agg_model as am
import bls12_381_model as m

pytestmark = pytest.mark.gpu
N_KEYS = 36
TOTAL = 36          # the row that holds the sum of the 36 keys
N_TABLE = 37


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def table():
    """(model points, rows (37, 12))"""
    _, pks = am.key_table(N_KEYS)
    total = None
    for p in pks:
        total = m.g1_add(total, p)
    pts = list(pks) + [total]
    return pts, am.table_rows(pts)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def run_dev(eng, rows, idx, seg_off, n_table=N_TABLE):
    """the _dev flavour on resident tensors with sentinels behind it: (out, inf, status) as numpy"""
    import torch
    a_idx, a_off = am.entry_arrays(idx, seg_off)
    out, inf, st = eng.g1_segment_sum(_dev(rows[:n_table]), _dev(a_idx), _dev(a_off))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), inf.cpu().numpy(), st.cpu().numpy()


def check(eng, table, idx, seg_off, host=True):
    pts, rows = table
    want = am.sum_rows(pts, idx, seg_off)
    got = run_dev(eng, rows, idx, seg_off)
    for g, w, what in zip(got, want, ("out", "out_inf", "status")):
        assert g.tobytes() == w.tobytes(), "_dev flavour: %s differs" % what
    if host:
        a_idx, a_off = am.entry_arrays(idx, seg_off)
        got = eng.g1_segment_sum(rows, a_idx, a_off)
        for g, w, what in zip(got, want, ("out", "out_inf", "status")):
            assert g.tobytes() == w.tobytes(), "host flavour: %s differs" % what
    return want


def _off(lens):
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    return off


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
    check(eng, table, _rows(33, 33), _off((1,) * 33))


@pytest.mark.parametrize("n_seg", [1, 63, 64, 65, 130])
def test_identities_at_the_borders_of_the_shared_inversion(eng, table, n_seg):
    """identities (an empty segment, a cancelling pair) at the first and the last lane of a wavefront, and at 130 sums the whole second
    wavefront: a zero Z that entered the shared product would zero every sum of its wavefront"""
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
    assert want[0].tolist() == am.g1_rows([m.g1_mul(pts[5], 40)])[0][0].tolist()
    check(eng, table, [5 | am.SIGN] * 40, _off((40,)))


def test_a_row_and_its_negative_cancel(eng, table):
    a, b = 3, 11
    idx = [a, a | am.SIGN, a, a | am.SIGN, b, a, b, a | am.SIGN, b | am.SIGN, a | am.SIGN, a]
    want, inf, _ = check(eng, table, idx, _off((2, 3, 4, 2)))
    assert inf.tolist() == [1, 0, 1, 1] and want[1].tobytes() == table[1][b].tobytes()


def test_the_total_minus_the_absent_is_the_sum_of_the_rest(eng, table):
    import zkvm_pairings_amd as z
    pts, rows = table
    x, y = 4, 29
    rest = None
    for r in range(N_KEYS):
        if r not in (x, y):
            rest = m.g1_add(rest, pts[r])
    idx, seg_off = z.committee_entries([[x, y], []], absent_from=TOTAL)
    assert idx.tolist() == [TOTAL, x | am.SIGN, y | am.SIGN, TOTAL]
    want, _, _ = check(eng, table, idx.tolist(), seg_off.tolist())
    assert want[0].tobytes() == am.g1_rows([rest])[0][0].tobytes() and want[1].tobytes() == rows[TOTAL].tobytes()
    got, inf = z.bls_aggregate_keys(rows, [[x, y], []], absent_from=TOTAL, engine=eng)
    assert got.tobytes() == want.tobytes() and not inf.any()
    every = z.bls_aggregate_keys(rows, [list(range(N_KEYS))], engine=eng)[0]
    assert every[0].tobytes() == rows[TOTAL].tobytes()


@pytest.mark.parametrize("row", [N_TABLE, 0x7FFFFFFF, N_TABLE | am.SIGN])
def test_a_row_beyond_the_table_refuses_its_segment_and_leaves_the_neighbours(eng, table, row):
    lens = (3, 40, 2)
    idx = _rows(sum(lens), 7)
    idx[3 + 17] = row
    want, inf, st = check(eng, table, idx, _off(lens), host=False)
    assert st.tolist() == [0, 1, 0] and inf.tolist() == [0, 1, 0] and want[1].tolist() == [0] * 6 + [1] + [0] * 5


MALFORMED = {"decreasing": [0, 5, 4, 45], "first-not-zero": [1, 5, 9, 45], "last-beyond": [0, 5, 9, 46], "last-below": [0, 5, 9, 44]}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_offsets_refuse_every_segment_and_raise_the_validation_word(kind):
    from zkvm_pairings_amd import PairingEngine
    _, pks = am.key_table(N_KEYS)
    rows = am.table_rows(pks)
    idx, off = _rows(45, 2), MALFORMED[kind]
    e = PairingEngine(0, validate=True)
    try:
        out, inf, st = run_dev(e, rows, idx, off, n_table=N_KEYS)
        assert st.tolist() == [1, 1, 1] and inf.tolist() == [1, 1, 1] and out.tobytes() == am.g1_rows([None] * 3)[0].tobytes()
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
    out, inf, st = np.full((3, 12), 7, dtype=np.uint64), np.full(3, 7, dtype=np.uint8), np.full(3, 7, dtype=np.uint8)

    def call(n_table, idx, off):
        a_idx, a_off = am.entry_arrays(idx, off)
        return eng._lib.zkp_g1_segment_sum_batch(eng._h, p(rows), n_table, p(a_idx) if a_idx.size else None, a_idx.size, p(a_off), len(off) - 1, p(out), p(inf),
                                                 p(st))
    idx = _rows(45, 2)
    for off in MALFORMED.values():
        assert call(N_TABLE, idx, off) == -1
    bad = list(idx)
    bad[44] = N_TABLE
    assert call(N_TABLE, bad, [0, 5, 9, 45]) == -1
    assert call(0, idx, [0, 5, 9, 45]) == -1                                        # entries and no table
    assert call((1 << 24) + 1, idx, [0, 5, 9, 45]) == -1
    assert eng._lib.zkp_g1_segment_sum_batch(eng._h, p(rows), N_TABLE, None, 45, p(out), 3, p(out), p(inf), p(st)) == -1
    assert (out == 7).all() and (inf == 7).all() and (st == 7).all()
    assert call(N_TABLE, idx, [0, 5, 9, 45]) == 0 and not st.any()
    assert call(0, [], [0, 0, 0, 0]) == 0 and inf.tolist() == [1, 1, 1]               # no table, no entries: three identities
