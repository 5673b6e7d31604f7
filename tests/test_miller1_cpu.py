"""CPU gate for the specialised Miller kernel of one-pair checks (k_miller1): the block tools/coopasm.py generate_miller1 emits is
executed by tools/asmemu.py on the twelve lanes of one check - prologue, the first three iterations (the first of them an addition
iteration), the closing line product and the state records, on a loop shortened to those iterations - and must leave, after every
MULACC body, the limbs tools/coopgen.py's emulator leaves when it runs the same steps of prog_miller(1, False)."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import asmemu  # noqa: E402
import coopasm  # noqa: E402
import coopgen as cg  # noqa: E402
import bls12_381_model as m  # noqa: E402

NL = 14
N_ITER = 3
LINES_AT, STATE_AT = 0x100000, 0x800000


def _flat(steps):
    out, i = [], 0
    while i < len(steps):
        st = steps[i]
        if st["op"] == cg.OP_LOOP:
            j = i + 1
            while steps[j]["op"] != cg.OP_ENDLOOP:
                j += 1
            out += steps[i + 1:j] * st["n"]
            i = j + 1
            continue
        out.append(st)
        i += 1
    return out


def _short_program():
    """the steps of prog_miller(1, False) for a loop of N_ITER iterations: prologue, the iterations, closing line product, output"""
    flat = _flat(cg.prog_miller(1, False).steps)
    assert [st["op"] for st in flat[:2]] == [cg.OP_LIN, cg.OP_LIN]
    n_sq, i = 0, 2
    while n_sq < N_ITER:
        n_sq += flat[i]["op"] == cg.OP_MULACC and flat[i]["T"] == 7
        i += 1
    tail = flat[-4:]
    assert [st["op"] for st in tail] == [cg.OP_GLOAD, cg.OP_MULACC, cg.OP_LIN, cg.OP_GSTORE]
    return flat[:i] + tail


def _model(lines):
    """per MULACC step of the short program: the accumulator and companion slots the step model leaves; the state records"""
    em = cg.Emu(lines=lines)
    after = []
    for st in _short_program():
        em.run([st])
        if st["op"] == cg.OP_MULACC:
            after.append([list(em.slot[s]) for s in range(24)])
    return after, [list(em.state[cg.ST_F + j]) for j in range(12)]


def _run_block(lines):
    bits = cg.miller_bits()[:N_ITER]
    assert bits[0], "the first iteration is an addition iteration"
    g = coopasm.generate_miller1(bits=bits)
    assert (g.S, g.SC) == (cg.LDS_WIDE_SLOTS, cg.LDS_WIDE_CONSTS) and g.n_line_steps == N_ITER + sum(bits) + 1
    p_limbs = [(cg.P >> (28 * i)) & 0xfffffff for i in range(NL)]
    subst = {"p%d" % i: v for i, v in enumerate(p_limbs)}
    subst.update({"pinv": (-pow(cg.P, -1, 1 << 28)) % (1 << 28), "act": "s[106:107]", "lines": "s[100:101]", "state": "s[110:111]", "stride": "s112"})
    emu = asmemu.Emu(lanes=12, subst=subst)
    n_checks = nc = 1
    emu.s[100], emu.s[101], emu.s[106], emu.s[107], emu.s[110], emu.s[111], emu.s[112] = LINES_AT, 0, 0xfff, 0, STATE_AT, 0, 6 * n_checks * 64
    PS = g.PS

    def put(idx, limbs):
        for i in range(16):
            emu.lds[16 * idx + (i // 4) * PS * 16 + 4 * (i % 4)] = (limbs[i] if i < NL else 0) & asmemu.M32

    # the image k_miller1 starts from: the program's constants, the operand table in the padding records
    consts = cg.Emu().slot
    for c in range(g.SC):
        put(c, consts[cg.CONST_BASE + c])
    for r, row in enumerate(g.rows):
        assert g.row_off[r] // 16 % PS >= g.SC + (r % 5) * g.SG + g.S, "a row lies in the padding behind a group's slots"
        for lig, ent in enumerate(row):
            for k in range(2):
                emu.lds[g.row_off[r] + 8 * lig + 4 * k] = ent[k] if ent else 0
    # the lane constants as the kernel derives them (group 0, check 0)
    gb = 16 * g.SC
    for lig in range(12):
        for reg, val in ((g.vtab, 8 * lig), (g.vgb, gb), (g.F, g.flags[lig]), (g.vdst, gb + 16 * lig),
                         (g.voff, ((lig >> 1) * n_checks + 0) * 64 + (lig & 1) * 32),
                         (g.vland, gb + 16 * (24 + (lig >> 1)) + (lig & 1) * 2 * PS * 16), (g.vst, (lig * nc + 0) * 64)):
            emu.v.setdefault(reg, [None] * 12)[lig] = val
    # the line stream: [(step * 1 + 0) * 6 + c][check] records of 16 words
    for s in range(g.n_line_steps):
        for c in range(6):
            limbs = cg.mont(lines[s][0][c])
            for i in range(16):
                emu.mem[LINES_AT + ((s * 6 + c) * n_checks + 0) * 64 + 4 * i] = (limbs[i] if i < NL else 0) & asmemu.M32
    seen = []

    def snap(e):
        def slot(s):
            return [asmemu.s32(e.lds[16 * (g.SC + s) + (i // 4) * PS * 16 + 4 * (i % 4)]) for i in range(NL)]
        regs = [[asmemu.s32(e.v[g.A[0] + i][lane]) for i in range(NL)] for lane in range(12)]
        seen.append(([slot(s) for s in range(24)], regs))

    emu.run(g.lines, max_steps=50_000_000, watch={".Lm1_done_l_%=": snap, ".Lm1_done_s_%=": snap})
    assert emu.exec == 0xfff
    state = [[asmemu.s32(emu.mem[STATE_AT + (j * nc + 0) * 64 + 4 * i]) for i in range(16)] for j in range(12)]
    return seen, state


def _compare(lines):
    want, want_state = _model(lines)
    seen, state = _run_block(lines)
    n_add = sum(cg.miller_bits()[:N_ITER])
    assert len(seen) == len(want) == N_ITER + n_add + N_ITER + 1      # line products (those of addition steps too), squarings, the closing product
    for k, ((slots, regs), w) in enumerate(zip(seen, want)):
        for lane in range(12):
            assert regs[lane] == w[lane], (k, lane, "the fourteen result limbs")
            assert slots[lane] == w[lane], (k, lane, "result slot")
            assert slots[12 + lane] == w[12 + lane], (k, lane, "companion slot")
    for j in range(12):
        assert state[j][:NL] == want_state[j] and state[j][NL:] == [0, 0], (j, "state record")
    return want


def test_block_equals_the_step_model_on_the_first_iterations():
    _compare(cg.model_lines([(m.G1_GEN, m.G2_GEN)]))


def test_neutral_line_stream_leaves_the_accumulator_at_one():
    want = _compare(cg.model_lines([(None, m.G2_GEN)]))
    for slots in want:
        assert [cg.from_mont(slots[j]) % cg.P for j in range(12)] == [1] + [0] * 11


def test_shared_emitters_still_generate_the_committed_blocks():
    csrc = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        coopasm.write_inc(os.path.join(td, "a.inc"))
        coopasm.write_miller1_inc(os.path.join(td, "b.inc"))
        assert open(os.path.join(td, "a.inc")).read() == open(os.path.join(csrc, "zkp_coop_mulacc.inc")).read(), "zkp_coop_mulacc.inc changed"
        assert open(os.path.join(td, "b.inc")).read() == open(os.path.join(csrc, "zkp_miller1.inc")).read(), \
            "zkp_miller1.inc is not what tools/coopasm.py generates: run tools/coopasm.py"
