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


# ------------------------------------------------------------------------------------------------------------------- k_grp_scale on what k_g1_mul_endo28 is tested on
M64 = (1 << 64) - 1
EDGE_PAIRS = [(1, 0), (0, 1), (M64, 0), (0, M64), (M64, M64), (1, 1), (M64, 1), (1, M64), (1 << 63, 1 << 63), (1 << 63, 0), (0, 0)]


def _same_rows(got, want, what):
    for g, w, name in zip(got, want, ("out", "out_inf", "status")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        assert g.tobytes() == w.tobytes(), "%s: %s differs, first at row %r" % (what, name, np.nonzero((g.view(np.uint8).reshape(len(w), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))[0][:1].tolist())


@pytest.mark.parametrize("flagged", [(), (0, 63)], ids=["no-flags", "flags-at-0-and-63"])
def test_one_entry_segments_on_the_edge_scalars_equal_the_model_and_g1_mul_endo(eng, table, flagged):
    """70 segments of one entry, a full wavefront of k_grp_scale and a short one: the scalars (a, b) with a or b 0, 1, 2^63 or 2^64 - 1, then
    seeded pairs.  out is the model's [a + b z^2] P and, row for row, what zkp_g1_mul_endo_batch gives; an input flagged at lane 0 or 63 is
    the identity"""
    n = 70
    rng = random.Random(70)
    picks = [rng.randrange(N_KEYS) for _ in range(n)]
    logs, pts, inf = _inputs(table, picks)
    rand = gm.rand_rows(n, 9)
    rand[:len(EDGE_PAIRS)] = np.array(EDGE_PAIRS, dtype=np.uint64)
    if 63 in flagged:
        rand[63] = (M64, M64)
    for j in flagged:
        logs[j], inf[j] = None, 1                                    # the words stay those of the table row: the flag decides
    _, oi, st = want = check(eng, logs, pts, inf if flagged else None, rand, list(range(n + 1)))
    assert np.nonzero(oi)[0].tolist() == sorted(set(flagged) | {EDGE_PAIRS.index((0, 0))}) and not st.any()
    endo, ei = eng.g1_mul_endo(pts, rand, inf if flagged else None)
    assert endo.tobytes() == want[0].tobytes() and ei.tobytes() == want[1].tobytes(), "g1_mul_endo"


def _outside_points():
    """points of E(Fp) outside G1: (0, +-2) of order 3, where phi'(P) = (beta x, -y) = -P and the table entry P + phi'(P) is the identity;
    a point of order 11; the fixture's points of small order and random points of the curve"""
    import h2g1_adversarial as ha
    import h2g1_model as g
    import outside_groups as og
    pts = [(0, 2), (0, g.P - 2), dict(ha.point_cases())["order11"]] + [q for q in og.g1_points().values() if g.e_on_curve(q)]
    out = []
    for q in pts:
        if q not in out:
            out.append(q)
    assert len(out) >= 6 and all(g.e_on_curve(q) and not g.in_g1(q) for q in out)
    return out


def _endo_value(q, a, b):
    """[a] P + [b] (beta x, -y) on all of E(Fp): what k_grp_scale's joint double-and-add computes whether or not P lies in G1"""
    import bls12_381_model as m
    import h2g1_model as g
    return g.e_add(g.e_mul(q, a), g.e_mul((q[0] * m.BETA % g.P, (-q[1]) % g.P), b))


def test_points_outside_g1_give_a_p_plus_b_phi_p_alone_and_three_to_a_segment(eng):
    import h2g1_model as g
    rng = random.Random(0xE0D3)
    rows, pairs = [], []
    for q in _outside_points():
        for a, b in [(1, 0), (0, 1), (1, 1), (M64, M64), (3, 5), (rng.getrandbits(64), rng.getrandbits(64))]:
            rows.append(q), pairs.append((a, b))
    n = len(rows)
    assert n % 3 == 0 and (rows[2], pairs[2]) == ((0, 2), (1, 1))
    pts = am.g1_rows(rows)[0]
    rand = np.array(pairs, dtype=np.uint64)
    vals = [_endo_value(q, a, b) for q, (a, b) in zip(rows, pairs)]
    assert vals[2] is None and vals[0] == (0, 2) and vals[1] == (0, g.P - 2)                    # T = P + phi'(P) is the identity; phi'(P) = -P
    singles = list(range(n + 1))
    want = am.g1_rows(vals) + (np.zeros(n, dtype=np.uint8),)
    _same_rows(run_dev(eng, pts, None, rand, singles), want, "_dev flavour, one entry per segment")
    _same_rows(eng.g1_scaled_segment_sum(pts, rand, gm.off_array(singles)), want, "host flavour, one entry per segment")
    endo, ei = eng.g1_mul_endo(pts, rand)
    assert endo.tobytes() == want[0].tobytes() and ei.tobytes() == want[1].tobytes(), "g1_mul_endo"
    triples = list(range(0, n + 1, 3))
    sums = [g.e_add(g.e_add(vals[i], vals[i + 1]), vals[i + 2]) for i in range(0, n, 3)]
    want = am.g1_rows(sums) + (np.zeros(n // 3, dtype=np.uint8),)
    assert sums[0] is None                                                                       # P + phi'(P) + the identity
    assert vals[3] is None and vals[4] == (0, 2)                                                 # [M64] (P - P); 3 P - 5 P = -2 P = P for a point of order 3
    _same_rows(run_dev(eng, pts, None, rand, triples), want, "_dev flavour, three entries per segment")


def test_equal_and_opposite_sums_that_meet_in_different_jacobian_representations(eng, table):
    """P1 = [s] g1 under (1, 0) and P2 = g1 under (a, b) with s = a + b z^2 are one point with two Z: [P1, P2] is the doubling branch of
    jac_add met by cross-multiplication, [-P1, P2] the cancellation, [P1, P2, Q] a chain after the doubling.  Once inside a run of 32
    records (level 0) and once across a run border, where the two meet as partial sums of the next level"""
    rng = random.Random(0x2A)
    n = 98
    picks = [rng.randrange(N_KEYS) for _ in range(n)]
    logs, pts, _ = _inputs(table, picks)
    rand = gm.rand_rows(n, 12)
    lens = [2, 2, 3, 24, 2, 30, 2, 30, 3]                            # the segments between the sites are whole ones of table rows
    off = _off(lens)
    sites = {0: False, 2: True, 4: False, 31: False, 63: True, 95: False}                      # where P1 stands; True: -P1
    assert off[-1] == n and set(sites) <= set(off) and all((at + 1) % 32 == 0 for at in (31, 63, 95))    # there P1 ends a run, P2 opens the next
    for at, neg in sites.items():
        a, b = (int(v) for v in gm.rand_rows(1, 100 + at)[0])
        s = gm.scalar(a, b)
        logs[at], logs[at + 1] = (gm.R - s if neg else s), 1
        rand[at], rand[at + 1] = (1, 0), (a, b)
        pts[at:at + 2] = gm.point_rows(logs[at:at + 2])[0]
    want = check(eng, logs, pts, None, rand, off)
    oi = want[1]
    assert [off[g] for g in np.nonzero(oi)[0]] == [2, 63] and not want[2].any()
    for start in (0, 31):                                                                        # [2 s] g1, stated from the scalar
        seg = off.index(start)
        a, b = gm.rand_pairs(rand)[start + 1]
        assert want[0][seg].tobytes() == am.g1_rows([am.public_key(2 * gm.scalar(a, b))])[0][0].tobytes()


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
