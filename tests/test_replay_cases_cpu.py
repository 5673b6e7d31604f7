"""No GPU: every `zkp_*_dev` entry point declared in include/zkp_pairings.h has either a replay case in tests/replay_cases.py or a
written reason why it has none, so that a device-pointer entry point added later cannot ship without one or the other."""
import os
import re

import replay_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    with open(os.path.join(ROOT, "include", "zkp_pairings.h")) as f:
        return set(re.findall(r"\b(zkp_\w+_dev)\(", f.read()))


def test_every_dev_entry_point_has_a_replay_case_or_a_written_reason():
    declared = _declared()
    table, excluded = rc.table_c_names(), set(rc.EXCLUDED)
    assert len(declared) >= 44
    assert not (table & excluded), sorted(table & excluded)
    assert declared - (table | excluded) == set(), "no replay case and no reason: %s" % sorted(declared - (table | excluded))
    assert (table | excluded) - declared == set(), "not declared in the header: %s" % sorted((table | excluded) - declared)
    assert all(isinstance(why, str) and len(why) > 20 for why in rc.EXCLUDED.values())


def test_the_table_is_well_formed():
    ids = [c.id for c in rc.CASES]
    assert len(ids) == len(set(ids))
    nodes = [c.nodes for c in rc.CASES]
    assert set(nodes) == {"kernel", "memset/copy"}
    assert nodes == sorted(nodes, key=lambda x: x != "kernel")                  # kernel-only graphs first
    from zkvm_pairings_amd.engine import PairingEngine
    for c in rc.CASES:
        assert c.c_names and callable(getattr(PairingEngine, c.method)), c.id
        assert len(c.shape) == len(c.small), c.id
