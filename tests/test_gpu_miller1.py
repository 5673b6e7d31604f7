"""GPU tests of k_miller1, the Miller loop of one-pair checks without the step interpreter: the fused pairing pass (Gt, ok bytes, flag)
on the new kernel equals, byte for byte, the same pass on the interpreter (ZKP_COOP_MILLER1=0; the knob is read when a context is
created, so two engines) and the CPU oracle."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as o
import outside_groups as og

pytestmark = pytest.mark.gpu

NTHREADS = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(monkeypatch, knob, chunk=None):
    from zkvm_pairings_amd import PairingEngine
    monkeypatch.setenv("ZKP_COOP_MILLER1", knob)
    if chunk:
        monkeypatch.setenv("ZKP_COOP_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("ZKP_COOP_CHUNK", raising=False)
    return PairingEngine(0)


@pytest.fixture(scope="module")
def pairs():
    """321 seeded pairs (every size below takes a prefix) and the oracle's pairings of the first 64"""
    from zkvm_pairings_amd import PairingEngine, synthetic
    e = PairingEngine(0)
    try:
        g1, g2, _, _ = synthetic.random_pairs(e, 321, seed=0x1117)
    finally:
        e.close()
    return g1, g2, o.pairing_batch(g1[:64], g2[:64], nthreads=NTHREADS)


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def _h(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _gt_check(eng, g1, g2, i1=None, i2=None):
    import torch
    n = g1.shape[0]
    out = torch.empty((n, 72), dtype=torch.int64, device="cuda:0")
    okt = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    allt = torch.ones(1, dtype=torch.int32, device="cuda:0")
    eng.pairing_gt_check(_t(g1), _t(g2), 1, out, okt, allt, None if i1 is None else _t(i1), None if i2 is None else _t(i2))
    return _h(out), _h(okt), int(_h(allt)[0])


def _both(monkeypatch, fn, chunk=None):
    """fn(engine) on the new kernel and on the interpreter"""
    res = []
    for knob in ("1", "0"):
        e = _engine(monkeypatch, knob, chunk)
        try:
            res.append(fn(e))
        finally:
            e.close()
    return res


@pytest.mark.parametrize("n", (1, 4, 5, 6, 59, 60, 61, 64, 321))
def test_fused_pass_equals_the_interpreter_and_the_oracle(monkeypatch, pairs, n):
    """one check; four (a lane group without a check in the only wavefront); one full wavefront; one wavefront and one lane group; 59
    (the last wavefront one check short), 60 (full), 61 (one over); 64; 321 in chunks of 320 (two pipelines, the second chunk of one check)"""
    g1, g2, want = pairs
    new, old = _both(monkeypatch, lambda e: _gt_check(e, g1[:n], g2[:n]), chunk=320 if n == 321 else None)
    assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1]) and new[2] == old[2]
    assert not new[1].any() and new[2] == 0
    if n <= 64:
        assert np.array_equal(new[0], want[:n])


def test_infinities_inside_a_wavefront(monkeypatch, pairs):
    """a G1 and a G2 infinity flag in checks 7 and 8 of the 64 (lane groups 2 and 3 of the second wavefront): identity, ok byte 1, the
    other checks of the wavefront untouched"""
    g1, g2, want = pairs
    i1, i2 = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    i1[7], i2[8] = 1, 1
    new, old = _both(monkeypatch, lambda e: _gt_check(e, g1[:64], g2[:64], i1, i2))
    assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1]) and new[2] == old[2] == 0
    one = o.fp12_one()
    for c in range(64):
        if c in (7, 8):
            assert np.array_equal(new[0][c], one) and new[1][c] == 1
        else:
            assert np.array_equal(new[0][c], want[c]) and new[1][c] == 0


def test_infinities_at_the_ends_of_a_launch_and_in_a_whole_wavefront(monkeypatch, pairs):
    """64 checks, thirteen wavefronts, the last with four checks: an infinity flag on check 0, on check 63 (the last check of the partial
    wavefront) and on all five checks of the third wavefront (10..14, G1 and G2 flags mixed, one check with both): identity and ok byte 1
    there, every other check untouched"""
    g1, g2, want = pairs
    i1, i2 = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    i1[0], i2[63] = 1, 1
    i1[[10, 12, 14]] = 1
    i2[[11, 13, 14]] = 1
    flagged = (0, 10, 11, 12, 13, 14, 63)
    new, old = _both(monkeypatch, lambda e: _gt_check(e, g1[:64], g2[:64], i1, i2))
    assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1]) and new[2] == old[2] == 0
    one = o.fp12_one()
    for c in range(64):
        if c in flagged:
            assert np.array_equal(new[0][c], one) and new[1][c] == 1, c
        else:
            assert np.array_equal(new[0][c], want[c]) and new[1][c] == 0, c


def test_one_engine_on_a_large_a_small_and_the_large_batch_again(monkeypatch, pairs):
    """64 checks, then 6, then the 64 again on ONE engine: during the second call the line buffer and the state buffer still hold the
    records of the first beyond check 5 (and the stride of the line buffer differs).  The third result is the first, the second is a
    fresh engine's, both are the oracle's - on the new kernel and on the interpreter"""
    g1, g2, want = pairs
    got = []
    for knob in ("1", "0"):
        e = _engine(monkeypatch, knob)
        try:
            runs = [_gt_check(e, g1[:n], g2[:n]) for n in (64, 6, 64)]
        finally:
            e.close()
        e = _engine(monkeypatch, knob)
        try:
            fresh = _gt_check(e, g1[:6], g2[:6])
        finally:
            e.close()
        for a, b in ((runs[2], runs[0]), (runs[1], fresh)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 0, knob
        assert np.array_equal(runs[0][0], want[:64]) and np.array_equal(runs[1][0], want[:6]) and not runs[0][1].any() and not runs[1][1].any(), knob
        got.append(runs)
    for a, b in zip(*got):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_g2_point_off_the_twist(monkeypatch, pairs):
    """check 3 of 11 takes a G2 point that is not on the twist (the line steps' second launch supplies its lines): the interpreter's
    bytes and the oracle's"""
    g1, g2, _ = pairs
    a, b = g1[:11].copy(), g2[:11].copy()
    b[3] = og.g2_wire(og.g2_points()["off_gen_y1"])
    new, old = _both(monkeypatch, lambda e: _gt_check(e, a, b))
    assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1]) and new[2] == old[2]
    assert np.array_equal(new[0], o.pairing_batch(a, b, nthreads=NTHREADS))


def test_device_resident_check_count(monkeypatch, pairs):
    """points_check on 12 uncompressed pairs, every third G1 off the curve: the Miller launch takes its check count from device memory"""
    import torch
    from zkvm_pairings_amd import configs
    g1, g2, _ = pairs
    raw1, raw2 = configs.to_bytes(g1[:12], 1), configs.to_bytes(g2[:12], 2)
    raw1[::3, 95] ^= 1          # y + 1 or y - 1: not on the curve

    def run(e):
        st1 = torch.empty(12, dtype=torch.uint8, device="cuda:0")
        st2 = torch.empty(12, dtype=torch.uint8, device="cuda:0")
        ok = torch.empty(12, dtype=torch.uint8, device="cuda:0")
        allt = torch.ones(1, dtype=torch.int32, device="cuda:0")
        e.points_check(_t(raw1), _t(raw2), 1, st1, st2, ok, allt)
        return _h(st1), _h(st2), _h(ok), int(_h(allt)[0])

    new, old = _both(monkeypatch, run)
    assert all(np.array_equal(x, y) for x, y in zip(new[:3], old[:3])) and new[3] == old[3] == 0
    assert (new[0] != 0).tolist() == [True, False, False] * 4 and not new[1].any() and not new[2].any()


def test_register_facts_of_the_new_kernel():
    so = os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    data = open(so, "rb").read()
    found = []
    for i in [m.start() for m in re.finditer(b"\x7fELF\x02\x01\x01", data)][1:]:       # the embedded gfx950 code objects (tests/test_codeobject.py)
        path = "/tmp/zkp_miller1_codeobject_%d.elf" % i
        with open(path, "wb") as f:
            f.write(data[i:])
        notes = subprocess.run([readelf, "--notes", path], capture_output=True, text=True).stdout
        os.unlink(path)
        for blk in notes.split("- .agpr_count")[1:]:
            nm = re.search(r"\.name:\s+(\S+)", blk)
            if nm and "9k_miller1E" in nm.group(1):
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                found.append((g("vgpr_count"), g("vgpr_spill_count"), g("private_segment_fixed_size")))
    assert len(found) == 1, found
    vgpr, spill, scratch = found[0]
    assert vgpr <= 168 and spill == 0 and scratch == 0, found
