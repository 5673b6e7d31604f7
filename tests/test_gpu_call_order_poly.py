"""Call-order independence of the calls of include/zkp_poly.h, zkp_prove.h and zkp_fk20.h on one MI355X (run with -m gpu), in the manner
of tests/test_gpu_call_order.py, whose helpers this module imports: every row of poly_replay_cases, prove_replay_cases and
fk20_replay_cases runs large, smallest, large, small, medium, smallest on a FRESH engine, on alternating flavours, each step on inputs of
its own against the row's own expected bytes (Python integers, one oracle multiplication per point).  Then the state these calls SHARE:
the one cached domain table (ctxop::kzg_domain) that the Fr NTT, fr_eval, the opening, the prover, the G1 NTT and FK20 all read and any of
them may rebuild, with the split-twiddle table that depends on it (ctxop::g1ntt_tables); fk20_ws, which the G1 NTT fills with records
from 0 and FK20 with records and then field elements; kzg_ws, prove_ws and msm_ws.  Each mixed sequence runs forward on one fresh engine
and in reverse on another."""
import pytest

import fk20_replay_cases as frc
import poly_model as pm
import poly_replay_cases as prc
import prove_replay_cases as pvc
import replay_cases as rc
from test_gpu_call_order import FLAVOURS, SEED, call, fresh, helper, same, sequence, to_dev  # noqa: F401  (helper: the fixture)

pytestmark = pytest.mark.gpu
ALL = pm.INVERSE | pm.BITREV | pm.COSET


def case_of(id):
    return [c for table in (rc.CASES, prc.CASES, pvc.CASES, frc.CASES) for c in table if c.id == id][0]


def run_sequence(helper, id, shapes):
    assert len(shapes) == len(FLAVOURS)
    eng = fresh()
    try:
        sequence(eng, helper, case_of(id), shapes)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------- one kind per engine
@pytest.mark.parametrize("flags", [0, ALL])
def test_fr_ntt_sizes(helper, flags):
    """2^13 takes a top pass through the workspace; the one-pass sizes after it, and 2^0 and 2^1, run in what it left"""
    run_sequence(helper, "fr_ntt-log12-x5-flags0", [(n, lg, flags) for n, lg in ((3, 13), (1, 0), (3, 13), (5, 4), (2, 11), (1, 1))])


@pytest.mark.parametrize("bitrev", [False, True])
def test_kzg_open_sizes(helper, bitrev):
    run_sequence(helper, "kzg_open-n3-N256%s" % ("-bitrev" if bitrev else ""), [(n, lg, bitrev) for n, lg in ((5, 9), (1, 0), (5, 9), (3, 2), (2, 6), (1, 0))])


@pytest.mark.parametrize("flags", [pm.BITREV, pm.INVERSE])
def test_g1_ntt_sizes(helper, flags):
    run_sequence(helper, "g1_ntt-N64-x3-flags%d" % flags, [(n, lg, flags) for n, lg in ((3, 8), (1, 0), (3, 8), (5, 2), (1, 6), (1, 0))])


def test_kzg_fk20_sizes(helper):
    run_sequence(helper, "kzg_fk20-n3-N64-bitrev", [(n, lg, True) for n, lg in ((3, 7), (1, 0), (3, 7), (2, 2), (1, 5), (1, 0))])


def test_kzg_fk20_setup_sizes(helper):
    run_sequence(helper, "kzg_fk20_setup-N64", [(lg,) for lg in (7, 0, 7, 2, 5, 0)])


@pytest.mark.parametrize("id", ["fr_spmv-n3-N64", "groth16_quotient-n3-N64", "groth16_prove-n3-N64"])
def test_prover_sizes(helper, id):
    """N = 4 is the smallest circuit the rows make (one row short of the domain, two entries per row)"""
    run_sequence(helper, id, [(3, 8), (1, 2), (3, 8), (2, 3), (1, 6), (1, 2)])


# ------------------------------------------------------------------------------------------------------------------- mixed kinds
def make_steps(helper, plan, base):
    """(case, shape, inputs, expected, flavour) per step: step i takes set i mod 3 of a build of its own seed"""
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


G1_FWD, G1_INV = "g1_ntt-N64-x3-flags%d" % pm.BITREV, "g1_ntt-N64-x3-flags%d" % pm.INVERSE
FK20, FK20_SETUP, PROVE = "kzg_fk20-n3-N64-bitrev", "kzg_fk20_setup-N64", "groth16_prove-n3-N64"
OPEN, OPEN_BR, FR_NTT = "kzg_open-n3-N256", "kzg_open-n3-N256-bitrev", "fr_ntt-log12-x5-flags0"

# the domain a step asks for is 2^log2_n, FK20's and its setup's 2^(log2_n + 1)
DOMAIN_PLAN = [
    (G1_FWD, (3, 3, pm.BITREV)),           # builds the table at 2^3 and the split table with it
    (FR_NTT, (2, 11, 0)),                  # grows the table to 2^11 through another kind of call
    (G1_INV, (3, 3, pm.INVERSE)),          # the split table must have been rebuilt: it is read with stride 2^8
    (FK20, (2, 4, True)),
    (OPEN, (2, 12, False)),                # grows the table to 2^12
    (FK20, (2, 4, True)),                  # the split table again, stride 2^7
    (FK20_SETUP, (2,)),
    ("fr_eval-log9-x3", (6, 2, False)),
    (PROVE, (1, 6)),
    (OPEN_BR, (3, 3, True)),
    (G1_INV, (2, 8, pm.INVERSE)),
]
G1_STEPS = (0, 2, 3, 5, 6, 10)


@pytest.fixture(scope="module")
def domain_steps(helper):
    return make_steps(helper, DOMAIN_PLAN, 500)


def test_domain_table_grown_by_one_kind_and_read_by_another(domain_steps):
    run_steps(domain_steps, "domain forward")


def test_domain_table_in_reverse_order(domain_steps):
    """the largest domains first: 2^8 of the G1 NTT, then 2^12 of the opening rebuilds both tables"""
    run_steps(domain_steps[::-1], "domain reverse")


def test_domain_table_largest_first_then_every_group_call_strided(helper, domain_steps):
    """fr_ntt at 2^13 first: every G1 NTT and FK20 call after it reads the table strided and rebuilds nothing"""
    first = make_steps(helper, [(FR_NTT, (3, 13, 0))], 550)
    run_steps(first + [domain_steps[i] for i in G1_STEPS], "domain largest first")


WORKSPACE_PLANS = {
    # fk20_ws: the G1 NTT lays records out from 0, FK20 records and then field elements at L.fr
    "fk20_ws": [(G1_FWD, (3, 8, pm.BITREV)), (FK20, (1, 2, True)), (G1_FWD, (1, 0, pm.BITREV)), (FK20, (3, 7, True)), (G1_INV, (5, 2, pm.INVERSE))],
    # kzg_ws is laid out per slice by the opening and per call by the verifier and the inversion; msm_ws and prove_ws under them
    "msm_ws-kzg_ws": [(OPEN, (5, 9, False)), ("kzg-n5", (65,)), ("g1_msm-m65-x2-shared", (65, 2, True)), (PROVE, (3, 6)), (OPEN_BR, (1, 0, True)),
                      ("fr_invert-n5", (4097,))],
}


@pytest.mark.parametrize("which", sorted(WORKSPACE_PLANS))
def test_kinds_that_share_a_workspace_in_either_order(helper, which):
    steps = make_steps(helper, WORKSPACE_PLANS[which], 600 + 50 * sorted(WORKSPACE_PLANS).index(which))
    run_steps(steps, which + " forward")
    run_steps(steps[::-1], which + " reverse")
