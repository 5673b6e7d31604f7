"""Every capturable device-pointer entry point, captured into a hipGraph and replayed repeatedly on changed inputs, on one MI355X (run
with -m gpu).  The cases, their three input sets A, B, C and the expected bytes come from tests/replay_cases.py (Python integers, the
construction of the inputs, the CPU oracle - never the library under test).  Per case: the eager call on A, the capture of the same call
on the same tensors (a recording proxy checks which `_dev` symbols it reached), five replays on A, A, B, C, A with every output filled
with a sentinel before and compared byte for byte after each, one eager call of a smaller shape, and a sixth replay on A.  A graph is
never replayed after a call that could have grown a workspace of its context, and everything runs on the current torch stream."""
import numpy as np
import pytest

import replay_cases as rc

pytestmark = pytest.mark.gpu
SEED = 0x6A9
REPLAYS = (0, 0, 1, 2, 0)        # the set in the buffers at each of the five replays: A, A, B, C, A


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    """the engine the inputs are made with (host-pointer calls only): it never captures, and the engine under test never sees a call
    that is not part of the protocol"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


class Recorder:
    """forwards every attribute of the loaded library and notes the `_dev` functions that get called"""

    def __init__(self, lib):
        self._lib, self.called = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith("_dev"):
            return fn

        def call(*args):
            self.called.append(name)
            return fn(*args)
        return call


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def load(bufs, host):
    import torch
    for name, t in bufs.items():
        a = np.ascontiguousarray(host[name])
        t.copy_(torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a))


def same(outs, want, what):
    assert len(outs) == len(want), what
    for i, (t, w) in enumerate(zip(outs, want)):
        got = t.cpu().numpy()
        assert got.nbytes == w.nbytes, (what, i, got.shape, w.shape)
        assert got.tobytes() == np.ascontiguousarray(w).tobytes(), "%s: output %d differs" % (what, i)


def sentinel(outs):
    for i, t in enumerate(outs):
        t.fill_(9 if i % 2 else 7)


def replay_protocol(eng, helper, case, make_small=True):
    import torch
    sets, want = case.make(helper, case.shape, SEED)
    small = case.make(helper, case.small, SEED + 1) if make_small else None
    assert all(set(s) == set(sets[0]) and all(np.asarray(s[x]).shape == np.asarray(sets[0][x]).shape for x in s) for s in sets)
    bufs = {name: to_dev(a) for name, a in sets[0].items()}
    outs = case.run(eng, bufs, case.shape)                       # eager: the workspaces reach the call's size before the capture
    torch.cuda.synchronize()
    same(outs, want[0], "%s eager" % case.id)
    graph = torch.cuda.CUDAGraph()
    real, rec = eng._lib, Recorder(eng._lib)
    eng._lib = rec
    try:
        with torch.cuda.graph(graph):
            gouts = case.run(eng, bufs, case.shape)
    finally:
        eng._lib = real
    assert sorted(set(rec.called)) == sorted(case.c_names), (case.id, rec.called)
    try:
        for i, s in enumerate(REPLAYS):
            load(bufs, sets[s])
            sentinel(gouts)
            graph.replay()
            torch.cuda.synchronize()
            same(gouts, want[s], "%s replay %d (set %s)" % (case.id, i + 1, "ABC"[s]))
        if small is not None:
            sbufs = {name: to_dev(a) for name, a in small[0][0].items()}
            souts = case.run(eng, sbufs, case.small)              # an ordinary, smaller call on the same context: no workspace grows
            torch.cuda.synchronize()
            same(souts, small[1][0], "%s eager small" % case.id)
        load(bufs, sets[0])
        sentinel(gouts)
        graph.replay()
        torch.cuda.synchronize()
        same(gouts, want[0], "%s replay 6 (set A, after a smaller eager call)" % case.id)
    finally:
        del graph


@pytest.mark.parametrize("case", rc.CASES, ids=[c.id for c in rc.CASES])
def test_captured_call_replays_on_changed_inputs(eng, helper, case):
    replay_protocol(eng, helper, case)


def test_validation_word_follows_the_replayed_data(helper):
    """validation mode under capture: the range check is part of the graph and ORs into the context's word on every replay - canonical A
    leaves it clear, B with one non-canonical limb in the LAST element sets it (once: the query clears it), A again leaves it clear"""
    import torch
    from zkvm_pairings_amd import PairingEngine
    n = 65
    e = PairingEngine(0, validate=True)
    try:
        fr = rc.FR[0]
        assert fr.id == "fr_op-mul-n65"
        fsets, fwant = fr.make(helper, (n,), SEED)
        pair = [c for c in rc.PAIRING if c.id == "pairing-n65-k1"][0]
        psets, pwant = pair.make(helper, (n, 1), SEED)
        bad_fr = {x: v.copy() for x, v in fsets[1].items()}
        bad_fr["b"][n - 1] = rc.fr_rows([rc.R])[0]                                  # r itself: the smallest value that is not canonical
        bad_pair = {x: v.copy() for x, v in psets[1].items()}
        bad_pair["g2"][n - 1, 18:24] = np.array([(rc.P >> (64 * i)) & rc.M64 for i in range(6)], dtype=np.uint64)     # y.c1 = p
        for case, sets, want, bad in ((fr, fsets, fwant, bad_fr), (pair, psets, pwant, bad_pair)):
            bufs = {name: to_dev(a) for name, a in sets[0].items()}
            outs = case.run(e, bufs, case.shape)
            torch.cuda.synchronize()
            same(outs, want[0], "%s eager" % case.id)
            assert e.take_validation_status() is False
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gouts = case.run(e, bufs, case.shape)
            try:
                for step, (host, expect_bad) in enumerate(((sets[0], False), (bad, True), (sets[0], False))):
                    load(bufs, host)
                    sentinel(gouts)
                    graph.replay()
                    assert e.take_validation_status() is expect_bad, (case.id, step)
                    assert e.take_validation_status() is False, (case.id, step)        # the query cleared the word
                    if not expect_bad:
                        same(gouts, want[0], "%s validated replay %d" % (case.id, step + 1))
            finally:
                del graph
    finally:
        e.close()
