"""The device-pointer entry points of include/zkp_bls_grouped.h captured into a hipGraph and replayed on changed inputs, by the protocol of
tests/test_gpu_graph_replay.py (imported, not copied): the eager call, the capture, five replays on the sets A, A, B, C, A with sentinels
in the outputs, a smaller eager call, a sixth replay.  The shapes are the smallest that take two accumulation levels (40 records); between
the sets the points, the scalars, the cuts of the segments and the verdict of the verifiers change.  The cases and their expected bytes:
tests/grp_replay_cases.py.  Run with -m gpu."""
import pytest

import grp_replay_cases as grc
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


@pytest.mark.parametrize("case", grc.CASES, ids=[c.id for c in grc.CASES])
def test_captured_grouped_calls_replay_on_changed_inputs(eng, helper, case):
    replay_protocol(eng, helper, case)
