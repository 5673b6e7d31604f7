"""Call-order independence of the calls of include/zkp_cells.h on one MI355X (run with -m gpu), in the manner of
tests/test_gpu_call_order_poly.py, whose helpers this module imports: every row of cells_replay_cases runs large, smallest, large, small,
medium, smallest on a FRESH engine, on alternating flavours, each step on inputs of its own against the row's own expected bytes.  Then
the state these calls SHARE with the older ones: the cached domain table and the split-twiddle table that depends on it, which FK20, the G1
NTT, the Fr NTT and the cell calls all read and any of them may rebuild; fk20_ws, which FK20 fills with records and field elements and the
cell proofs with blocks of records, partials and field elements; kzg_ws and msm_ws, which the two verifiers lay out differently.  Each mixed
sequence runs forward on one fresh engine and in reverse on another."""
import pytest

import cells_replay_cases as crc
import poly_model as pm
from test_gpu_call_order import FLAVOURS, SEED, call, fresh, helper, sequence  # noqa: F401  (helper: the fixture)
from test_gpu_call_order_poly import case_of as older_case_of

pytestmark = pytest.mark.gpu
CELLS, CELLS_SETUP, VERIFY = [c.id for c in crc.CASES if c.method == "kzg_cells"][0], "kzg_cells_setup-N64-l4", "kzg_cell_verify-n5-N16-l4"
FK20, FK20_SETUP, G1_INV, FR_NTT, KZG = "kzg_fk20-n3-N64-bitrev", "kzg_fk20_setup-N64", "g1_ntt-N64-x3-flags%d" % pm.INVERSE, "fr_ntt-log12-x5-flags0", "kzg-n5"


def case_of(id):
    mine = [c for c in crc.CASES if c.id == id]
    return mine[0] if mine else older_case_of(id)


def run_sequence(helper, id, shapes):
    assert len(shapes) == len(FLAVOURS)
    eng = fresh()
    try:
        sequence(eng, helper, case_of(id), shapes)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------- one kind per engine
@pytest.mark.parametrize("bitrev", [False, True])
def test_kzg_cells_sizes(helper, bitrev):
    """(n, log2_n, log2_l, log2_ext): N = 128 with cells of 4, the smallest call there is (one coefficient, one cell), partials (g = 1 < l)
    and none (l = 1), both extensions"""
    run_sequence(helper, CELLS, [(3, 7, 2, 1, bitrev), (1, 0, 0, 0, bitrev), (3, 7, 2, 1, bitrev), (2, 2, 1, 1, bitrev), (1, 5, 0, 0, bitrev), (1, 0, 0, 1, bitrev)])


def test_kzg_cells_setup_sizes(helper):
    run_sequence(helper, CELLS_SETUP, [(7, 2), (0, 0), (7, 2), (2, 1), (5, 5), (0, 0)])


def test_kzg_cell_verify_sizes(helper):
    """(n, log2_n, log2_l, log2_ext, bitrev): 33 cells of 8 values, one cell of one value, ..."""
    run_sequence(helper, VERIFY, [(33, 5, 3, 1, True), (1, 0, 0, 0, True), (33, 5, 3, 1, True), (5, 2, 1, 1, False), (9, 4, 2, 0, True), (1, 0, 0, 1, False)])


# ------------------------------------------------------------------------------------------------------------------- mixed kinds
def make_steps(helper, plan, base):
    steps = []
    for i, (id, shape) in enumerate(plan):
        case = case_of(id)
        sets, want = case.make(helper, shape, SEED + base + i)
        steps.append((case, shape, sets[i % 3], want[i % 3], ("dev", "host")[i % 2]))
    return steps


def run_steps(steps, name):
    eng = fresh()
    try:
        for n, (case, shape, host, want, fl) in enumerate(steps):
            call(eng, case, shape, host, want, fl, "%s step %d: %s" % (name, n, case.id))
    finally:
        eng.close()


PLANS = {
    # the domain a cell call asks for is 2^(log2_n - log2_l + 1), the verifier's 2^log2_d, FK20's 2^(log2_n + 1)
    "domain": [(CELLS, (2, 4, 1, 1, True)),            # builds the table at 2^4 and the split table with it
               (FR_NTT, (2, 11, 0)),                   # grows the table to 2^11 through another kind of call
               (CELLS, (2, 4, 1, 1, True)),            # the split table must have been rebuilt: it is read with stride 2^7
               (FK20, (2, 4, True)),
               (VERIFY, (5, 4, 2, 1, True)),           # reads c^-i from the table of 2^11 with stride 2^6
               (CELLS_SETUP, (6, 2)),
               (G1_INV, (2, 8, pm.INVERSE)),
               (CELLS, (1, 6, 2, 0, False))],
    # fk20_ws: FK20 lays out records and then field elements, the cell proofs blocks of records, partials, field elements
    "fk20_ws": [(FK20, (3, 7, True)), (CELLS, (1, 2, 1, 1, True)), (CELLS, (3, 7, 2, 1, True)), (FK20, (1, 2, True)), (CELLS_SETUP, (7, 2)),
                (FK20_SETUP, (2,)), (CELLS, (2, 6, 0, 1, False))],
    # kzg_ws and msm_ws under the two verifiers
    "msm_ws-kzg_ws": [(VERIFY, (33, 5, 3, 1, True)), (KZG, (65,)), (VERIFY, (2, 2, 1, 1, True)), (KZG, (2,)), (VERIFY, (9, 4, 2, 0, False))],
}


@pytest.mark.parametrize("which", sorted(PLANS))
def test_state_shared_with_the_older_calls_in_either_order(helper, which):
    steps = make_steps(helper, PLANS[which], 700 + 50 * sorted(PLANS).index(which))
    run_steps(steps, which + " forward")
    run_steps(steps[::-1], which + " reverse")
