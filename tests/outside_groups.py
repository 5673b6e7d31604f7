"""The points of tests/golden/outside_groups.json (written by tests/golden/gen_fixtures.py from the big-integer model): on-curve points
of small order and random points outside the prime-order subgroups, and points off the curves, for G1 and the twist.  The pairing
entry points accept them (they ask only for canonical limbs); every pairing-shaped call must still compute
final_exponentiation(multi_miller_loop(..)) of the Alg. 26 / 27 formulas on them.  TEST INFRASTRUCTURE ONLY."""
import json
import os

import numpy as np

import bls12_381_model as m

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outside_groups.json")
_data = None


def data():
    global _data
    if _data is None:
        with open(PATH) as f:
            _data = json.load(f)
    return _data


def _ints(hexes):
    return [int(h, 16) for h in hexes]


def g1_points():
    """name -> (x, y); the fixture classes in file order"""
    return {k: tuple(_ints(v["p"])) for k, v in data()["g1"].items()}


def g2_points():
    """name -> ((x.c0, x.c1), (y.c0, y.c1))"""
    out = {}
    for k, v in data()["g2"].items():
        a = _ints(v["p"])
        out[k] = ((a[0], a[1]), (a[2], a[3]))
    return out


def g1_all():
    return dict(g1_points(), gen=m.G1_GEN)


def g2_all():
    return dict(g2_points(), gen=m.G2_GEN)


def g1_wire(p):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for v in p for i in range(6)], dtype=np.uint64)


def g2_wire(q):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for c in q for v in c for i in range(6)], dtype=np.uint64)


def f12_wire(ints12):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for v in ints12 for i in range(6)], dtype=np.uint64)
