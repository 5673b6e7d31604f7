"""zkp_g1_scaled_segment_sum_batch on one MI355X through the C ABI (run with -m gpu).  The points are rows of ONE table of 36 model keys
(tests/agg_model.py), so the model (tests/grp_model.py) knows their discrete logarithms and a sum of scaled points is one multiple of the
generator on Python integers.  out, out_inf and status are compared byte for byte, in the host flavour and in the _dev flavour.  The shapes
are the smallest that reach each path of the run-wise sum (runs of 32 records, two partials per run and level) and of the shared inversion
(wavefronts of 64 sums)."""
import ctypes
import random

import numpy as np
import pytest

import agg_model as am
import grp_model as gm

pytestmark = pytest.mark.gpu
N_KEYS = 36


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def table():
    """(secret keys, rows (36, 12))"""
    sks, pks = am.key_table(N_KEYS)
    return sks, am.table_rows(pks)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _off(lens):
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    return off


def _inputs(table, picks, negate=()):
    """picks[i]: a table row, or None for an input at infinity -> (logs, pts (n, 12), inf (n,)); rows in `negate` enter as -P"""
    sks, rows = table
    logs = [None if r is None else (gm.R - sks[r] if i in negate else sks[r]) for i, r in enumerate(picks)]
    pts = np.zeros((len(picks), 12), dtype=np.uint64)
    inf = np.zeros(len(picks), dtype=np.uint8)
    for i, r in enumerate(picks):
        if r is None:
            pts[i, 6], inf[i] = 1, 1
        else:
            pts[i] = rows[r]
            if i in negate:
                pts[i] = am.g1_rows([am.public_key(logs[i])])[0][0]
    return logs, pts, inf


def run_dev(eng, pts, inf, rand, seg_off):
    import torch
    out, oi, st = eng.g1_scaled_segment_sum(_dev(pts), _dev(rand), _dev(gm.off_array(seg_off)), inf=None if inf is None else _dev(inf))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), oi.cpu().numpy(), st.cpu().numpy()


def check(eng, logs, pts, inf, rand, seg_off, host=True):
    want = gm.sum_rows(logs, gm.rand_pairs(rand), seg_off)
    got = run_dev(eng, pts, inf, rand, seg_off)
    for g, w, what in zip(got, want, ("out", "out_inf", "status")):
        assert g.tobytes() == w.tobytes(), "_dev flavour: %s differs" % what
    if host:
        got = eng.g1_scaled_segment_sum(pts, rand, gm.off_array(seg_off), inf=inf)
        for g, w, what in zip(got, want, ("out", "out_inf", "status")):
            assert g.tobytes() == w.tobytes(), "host flavour: %s differs" % what
    return want


def test_one_two_and_three_levels_run_borders_and_the_inputs_that_contribute_nothing(eng, table):
    """1, 0, 2, 31, 32, 33, 0, 513: segments inside a run, across run borders, of one, two and three accumulation levels (513 records leave
    34 partials and then 4); an input at infinity, a row with a = 0, one with b = 0 and one with both zero"""
    lens = [1, 0, 2, 31, 32, 33, 0, 513]
    n = sum(lens)
    rng = random.Random(612)
    picks = [rng.randrange(N_KEYS) for _ in range(n)]
    picks[40] = None                                     # an input at infinity inside the segment of 32
    logs, pts, inf = _inputs(table, picks)
    rand = gm.rand_rows(n, 3)
    rand[5, 0] = 0                                       # a = 0
    rand[70, 1] = 0                                      # b = 0
    rand[200] = 0                                        # both: the point contributes nothing, which is no error here
    rand[1] = 0                                          # ... also when it is a segment's only other member
    _, oi, st = check(eng, logs, pts, inf, rand, _off(lens))
    assert oi.tolist() == [0, 1, 0, 0, 0, 0, 1, 0] and not st.any()


def test_p_and_minus_p_under_one_scalar_cancel(eng, table):
    picks = [3, 3, 9, 3, 3, 9]
    logs, pts, inf = _inputs(table, picks, negate={1, 4})
    rand = gm.rand_rows(6, 8)
    rand[1], rand[4] = rand[0], rand[3]
    _, oi, _ = check(eng, logs, pts, inf, rand, [0, 2, 3, 6])
    assert oi.tolist() == [1, 0, 0]
    _, oi, _ = check(eng, logs[:2], pts[:2], inf[:2], rand[:2], [0, 2])
    assert oi.tolist() == [1]


def test_one_point_and_scalar_forty_times_is_a_doubling_and_then_a_chain(eng, table):
    """the same (P, a, b) 40 times across a run border: the first addition of the accumulation is the doubling branch of jac_add"""
    sks, _ = table
    picks = [7] * 40 + [2]
    logs, pts, inf = _inputs(table, picks)
    rand = gm.rand_rows(41, 4)
    rand[:40] = rand[0]
    want, _, _ = check(eng, logs, pts, inf, rand, [0, 40, 41])
    r = gm.scalar(*gm.rand_pairs(rand)[0])
    assert want[0].tobytes() == am.g1_rows([am.public_key(40 * r * sks[7])])[0][0].tobytes()


def test_identities_at_the_borders_of_the_shared_inversion(eng, table):
    """65 sums, those at 0, 63 and 64 the identity (empty, cancelling, zero scalar): a zero Z that entered the shared product would zero
    every sum of its wavefront"""
    lens = [0] + [1 + j % 3 for j in range(1, 63)] + [2, 1]
    rng = random.Random(65)
    picks = [rng.randrange(N_KEYS) for _ in range(sum(lens))]
    off = _off(lens)
    picks[off[63] + 1] = picks[off[63]]
    logs, pts, inf = _inputs(table, picks, negate={off[63] + 1})
    rand = gm.rand_rows(len(picks), 6)
    rand[off[63] + 1] = rand[off[63]]
    rand[off[64]] = 0
    _, oi, st = check(eng, logs, pts, inf, rand, off)
    assert [j for j in range(65) if oi[j]] == [0, 63, 64] and not st.any()


MALFORMED = {"decreasing": [0, 5, 4, 45], "first-not-zero": [1, 5, 9, 45], "last-beyond": [0, 5, 9, 46], "last-below": [0, 5, 9, 44]}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_offsets_give_identities_with_status_one_and_touch_no_neighbour(table, kind):
    """the outputs are the middle rows of larger buffers: the guard rows around them keep their bytes"""
    import torch
    from zkvm_pairings_amd import PairingEngine
    rng = random.Random(45)
    logs, pts, _ = _inputs(table, [rng.randrange(N_KEYS) for _ in range(45)])
    rand, off = gm.rand_rows(45, 2), MALFORMED[kind]
    identity = am.g1_rows([None] * 3)[0]
    for validate in (True, False):
        e = PairingEngine(0, validate=validate)
        try:
            out = torch.full((5, 12), 0x55, dtype=torch.int64, device="cuda")
            oi, st = torch.full((5,), 0x55, dtype=torch.uint8, device="cuda"), torch.full((5,), 0x55, dtype=torch.uint8, device="cuda")
            p = lambda t, skip=0: ctypes.c_void_p(t.data_ptr() + skip)
            d_pts, d_rand, d_off = _dev(pts), _dev(rand), _dev(gm.off_array(off))
            rc = e._lib.zkp_g1_scaled_segment_sum_batch_dev(e._h, p(d_pts), None, p(d_rand), 45, p(d_off), 3, p(out, 96), p(oi, 1), p(st, 1), e._stream())
            torch.cuda.synchronize()
            assert rc == 0
            out, oi, st = out.cpu().numpy().view(np.uint64), oi.cpu().numpy(), st.cpu().numpy()
            assert out[1:4].tobytes() == identity.tobytes() and oi[1:4].tolist() == [1, 1, 1] and st[1:4].tolist() == [1, 1, 1]
            assert (out[[0, 4]] == 0x55).all() and oi[[0, 4]].tolist() == [0x55] * 2 and st[[0, 4]].tolist() == [0x55] * 2
            assert e.take_validation_status() is validate
            got = run_dev(e, pts, None, rand, [0, 5, 9, 45])                                 # the next call is not tainted
            want = gm.sum_rows(logs, gm.rand_pairs(rand), [0, 5, 9, 45])
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and e.take_validation_status() is False
        finally:
            e.close()


def test_the_host_flavour_refuses_what_it_can_see(eng, table):
    rng = random.Random(45)
    logs, pts, _ = _inputs(table, [rng.randrange(N_KEYS) for _ in range(45)])
    rand = gm.rand_rows(45, 2)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    out, oi, st = np.full((3, 12), 7, dtype=np.uint64), np.full(3, 7, dtype=np.uint8), np.full(3, 7, dtype=np.uint8)
    call = lambda n, off, n_seg=3: eng._lib.zkp_g1_scaled_segment_sum_batch(eng._h, p(pts), None, p(rand), n, p(gm.off_array(off)), n_seg, p(out), p(oi), p(st))
    for off in MALFORMED.values():
        assert call(45, off) == -1
    assert call((1 << 24) + 1, [0, 5, 9, 45]) == -1 and call(45, [0, 5, 9, 45], (1 << 24) + 1) == -1
    assert eng._lib.zkp_g1_scaled_segment_sum_batch(eng._h, p(pts), None, None, 45, p(gm.off_array([0, 5, 9, 45])), 3, p(out), p(oi), p(st)) == -1
    assert eng._lib.zkp_g1_scaled_segment_sum_batch(eng._h, p(pts), None, p(rand), 45, None, 3, p(out), p(oi), p(st)) == -1
    assert (out == 7).all() and (oi == 7).all() and (st == 7).all()
    assert call(45, [0, 5, 9, 45]) == 0 and not st.any() and not oi.any()
    assert call(0, [0, 0, 0, 0]) == 0 and oi.tolist() == [1, 1, 1]                            # no point: three identities
