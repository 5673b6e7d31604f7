"""Call-order independence of zkp_das_recover_batch on one MI355X (run with -m gpu), in the manner of tests/test_gpu_call_order_cells.py,
whose helpers this module imports: the recovery runs large, smallest, large, small, medium, smallest on a FRESH engine, on alternating
flavours, each step on inputs of its own against its own expected bytes.  Then the state it SHARES with older calls: the cached domain
table (the Fr NTT, the cell producer and the cell verifier read it and any of them may rebuild it at another size), the coset tables
(the Fr NTT builds them on its first coset call, the recovery on its first call), and kzg_ws, the workspace the recovery borrows - the
batched inversion, the barycentric evaluation, the KZG verifier and the cell verifier lay it out differently.  Each mixed sequence runs
forward on one fresh engine and in reverse on another; every answer is checked."""
import pytest

import poly_model as pm
import recover_replay_cases as rrc
from test_gpu_call_order import FLAVOURS, SEED, call, fresh, helper, sequence  # noqa: F401  (helper: the fixture)
from test_gpu_call_order_cells import case_of as older_case_of

pytestmark = pytest.mark.gpu
RECOVER = rrc.CASES[0].id
CELLS, VERIFY, KZG = "kzg_cells-n3-N64-l4-e2-bitrev", "kzg_cell_verify-n5-N16-l4", "kzg-n5"
FR_NTT, FR_NTT_COSET, FR_INVERT, FR_EVAL = "fr_ntt-log12-x5-flags0", "fr_ntt-log12-x5-flags%d" % (pm.BITREV | pm.COSET), "fr_invert-n1025", "fr_eval-log9-x3"


def case_of(id):
    mine = [c for c in rrc.CASES if c.id == id]
    return mine[0] if mine else older_case_of(id)


@pytest.mark.parametrize("bitrev", [False, True])
def test_recover_sizes(helper, bitrev):
    """(n, log2_n, log2_l): 5 blobs of 256 coefficients in cells of 8 (M = 64), the smallest call there is (one coefficient, two cells of
    one value), the large one again, a small one, one with a full tile column (M = 1024) and no cell transform, the smallest again"""
    shapes = [(5, 8, 3, bitrev), (1, 0, 0, bitrev), (5, 8, 3, bitrev), (2, 2, 1, bitrev), (1, 9, 0, bitrev), (1, 0, 0, bitrev)]
    assert len(shapes) == len(FLAVOURS)
    eng = fresh()
    try:
        sequence(eng, helper, case_of(RECOVER), shapes)
    finally:
        eng.close()


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
    # the recovery asks for the table of D = 2^(log2_n + 1) points and reads it with two strides
    "domain": [(RECOVER, (2, 4, 2, True)),             # builds the table at 2^5
               (FR_NTT, (2, 11, 0)),                   # grows it to 2^11 through another kind of call
               (RECOVER, (2, 4, 2, True)),             # now read with strides 2^6 and 2^8
               (CELLS, (2, 4, 1, 1, True)),
               (VERIFY, (5, 4, 2, 1, True)),
               (RECOVER, (1, 6, 0, False)),
               (FR_NTT, (1, 3, pm.INVERSE)),
               (RECOVER, (3, 7, 3, True))],
    # the coset tables: built by whichever call comes first
    "coset": [(RECOVER, (2, 4, 2, True)), (FR_NTT_COSET, (2, 6, pm.COSET)), (RECOVER, (1, 5, 1, False)), (FR_NTT_COSET, (1, 11, pm.COSET | pm.INVERSE))],
    # kzg_ws under its five tenants
    "kzg_ws": [(RECOVER, (5, 8, 3, True)), (FR_INVERT, (1025,)), (RECOVER, (1, 1, 1, False)), (VERIFY, (33, 5, 3, 1, True)), (RECOVER, (2, 4, 2, False)),
               (FR_EVAL, (9, 3, False)), (KZG, (5,)), (RECOVER, (5, 8, 3, False))],
}


@pytest.mark.parametrize("which", sorted(PLANS))
def test_state_shared_with_the_older_calls_in_either_order(helper, which):
    steps = make_steps(helper, PLANS[which], 900 + 50 * sorted(PLANS).index(which))
    run_steps(steps, which + " forward")
    run_steps(steps[::-1], which + " reverse")
