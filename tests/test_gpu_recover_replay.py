"""The device-pointer entry point of include/zkp_recover.h captured into a hipGraph and replayed on changed inputs, by the protocol of
tests/test_gpu_graph_replay.py (imported, not copied): the eager call, the capture, five replays on the sets A, A, B, C, A with
sentinels in the outputs, a smaller eager call, a sixth replay.  Between the sets the polynomials AND the erasure patterns change - the
vanishing polynomial, its two tables and the flags are recomputed inside the graph.  The cases and their expected bytes:
tests/recover_replay_cases.py.  Run with -m gpu."""
import pytest

import recover_replay_cases as rrc
from test_gpu_graph_replay import replay_protocol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", rrc.CASES, ids=[c.id for c in rrc.CASES])
def test_captured_recovery_replays_on_changed_inputs_and_patterns(eng, helper, case):
    sets, _ = case.make(helper, case.shape, 0)
    assert len({s["present"].tobytes() for s in sets}) == 3               # the erasure pattern is part of what changes
    replay_protocol(eng, helper, case)
