"""The device-pointer entry points of include/zkp_bls.h captured into a hipGraph and replayed on changed inputs, by the protocol of
tests/test_gpu_graph_replay.py (imported, not copied): the eager call, the capture, five replays on the sets A, A, B, C, A with sentinels
in the outputs, a smaller eager call, a sixth replay.  Between the sets the messages, their lengths (the offsets) and the verdict of the
verifier change.  The cases and their expected bytes: tests/bls_replay_cases.py.  Run with -m gpu."""
import pytest

import bls_replay_cases as brc
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


@pytest.mark.parametrize("case", brc.CASES, ids=[c.id for c in brc.CASES])
def test_captured_bls_calls_replay_on_changed_inputs(eng, helper, case):
    replay_protocol(eng, helper, case)
