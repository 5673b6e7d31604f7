"""The device-pointer entry points of include/zkp_bls_agg_g2.h captured into a hipGraph and replayed on changed inputs, by the protocol
of tests/test_gpu_graph_replay.py (imported, not copied): the eager call, the capture, five replays on the sets A, A, B, C, A with
sentinels in the outputs, a smaller eager call, a sixth replay.  The sums and the committee verifier run the smallest shape that takes two
accumulation levels (40 entries); AggregateVerify runs three signatures over nine messages.  Between the sets the rows, the signs, the
cuts of the segments (the offsets) and the verdicts change; set B of the sums holds a row beyond the table, set B of AggregateVerify two
signatures that changed places.  The cases and their expected bytes: tests/agg_g2_replay_cases.py.  Run with -m gpu."""
import pytest

import agg_g2_replay_cases as arc
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


@pytest.mark.parametrize("case", arc.CASES, ids=[c.id for c in arc.CASES])
def test_captured_g2_aggregation_calls_replay_on_changed_inputs(eng, helper, case):
    replay_protocol(eng, helper, case)
