"""CPU gate for the specialised Miller kernel of one-pair checks (k_miller1): the block tools/coopasm.py generate_miller1 emits is
executed by tools/asmemu.py (memory counters and wait states checked) and must leave, after every MULACC body, the limbs
tools/coopgen.py's emulator leaves when it runs the same steps of prog_miller(1, False).

  * twelve lanes of one check, loop shortened to three iterations (the first an addition iteration): the first three tests;
  * twelve lanes, the WHOLE loop (62 iterations, 68 line steps): on two pairs, with the state records raised through the big-integer
    model's final exponentiation to the pairing; on synthetic line streams of adversarial field values;
  * the whole wavefront (sixty lanes, three iterations): blocks other than the first, inactive lane groups on stale registers,
    nc != n_checks, st_off != 0 - every global and LDS access accounted for.  The lane constants come from the kernel's own header
    (zkp_miller1_lanes.hpp) through tests/miller1_plan_check.cpp, a stand-alone program built with ASan and UBSan."""
import os
import random
import re
import subprocess
import sys
import tempfile

import pytest

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


def _short_program(n_iter=N_ITER):
    """the steps of prog_miller(1, False) for a loop of n_iter iterations: prologue, the iterations, closing line product, output"""
    flat = _flat(cg.prog_miller(1, False).steps)
    assert [st["op"] for st in flat[:2]] == [cg.OP_LIN, cg.OP_LIN]
    n_sq, i = 0, 2
    while n_sq < n_iter:
        n_sq += flat[i]["op"] == cg.OP_MULACC and flat[i]["T"] == 7
        i += 1
    tail = flat[-4:]
    assert [st["op"] for st in tail] == [cg.OP_GLOAD, cg.OP_MULACC, cg.OP_LIN, cg.OP_GSTORE]
    assert n_iter < len(cg.miller_bits()) or flat[i:] == tail
    return flat[:i] + tail


def _model(lines, n_iter=N_ITER):
    """per MULACC step of the short program: the accumulator and companion slots the step model leaves; the state records"""
    em = cg.Emu(lines=lines)
    after = []
    for st in _short_program(n_iter):
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


# ================================================================================================ the whole block
# One runner for everything below: any number of lanes, any block of any launch.  The lane constants are the kernel's own
# (zkp_miller1_lanes.hpp, printed by tests/miller1_plan_check.cpp), the memory image is what k_miller1 and k_prep_lines set up.
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
ALL_BITS = cg.miller_bits()


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("miller1_plan") / "miller1_plan_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         "-o", exe, os.path.join(ROOT, "tests", "miller1_plan_check.cpp")], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _clean(out):
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]


def _lane_constants(plan_exe, block, n_checks, nc, st_off):
    """(stride, [per lane: dict grp lig check active vgb vdst vtab voff vland vst]) as the kernel computes them"""
    out = subprocess.run([plan_exe] + [str(x) for x in (block, n_checks, nc, st_off)], capture_output=True, text=True, timeout=60)
    _clean(out)
    rows = out.stdout.split("\n")
    assert rows[0].startswith("stride ") and rows[1] == "eligible 1"
    names = "lane grp lig check active vgb vdst vtab voff vland vst".split()
    lanes = [dict(zip(names, (int(x) for x in r.split()))) for r in rows[2:] if r]
    assert [c["lane"] for c in lanes] == list(range(60))
    return int(rows[0].split()[1]), lanes


class _Recorder(dict):
    """global memory that remembers what was read (how often) and what was written"""

    def __init__(self):
        super().__init__()
        self.reads, self.writes, self.armed = {}, set(), False

    def __getitem__(self, k):
        if self.armed:
            self.reads[k] = self.reads.get(k, 0) + 1
        return super().__getitem__(k)

    def __setitem__(self, k, v):
        if self.armed:
            self.writes.add(k)
        super().__setitem__(k, v)


class _WaveEmu(asmemu.Emu):
    """every LDS word a lane writes lies in the slots of the lane's own group (never in the constants, another group or the
    padding records, which hold the operand table)"""

    def _own(self, a, m, nbytes):
        g = self.geom
        for lane in range(self.n):
            if (self.exec >> lane) & 1:
                addr = self.rd(a[0], lane) + m.get("offset", 0)
                for rec in {addr // 16, (addr + nbytes - 1) // 16}:
                    plane, slot = divmod(rec, g.PS)
                    assert plane < 4 and 0 <= slot - (g.SC + (lane // 12) * g.SG) < g.S, "lane %d writes LDS record %d (plane %d, slot %d)" % (lane, rec, plane, slot)

    def op_ds_write_b64(self, a, m):
        self._own(a, m, 8)
        super().op_ds_write_b64(a, m)

    def op_ds_write_b128(self, a, m):
        self._own(a, m, 16)
        super().op_ds_write_b128(a, m)


def _run(bits, lanes, consts, stride, lines_of, n_checks, nc, st_off=0, stale=None, trace=None, mutate=None):
    """the block for the loop `bits` on the first `lanes` lanes of a wavefront whose lane constants are `consts`.
    lines_of: {check: line stream} for the checks of this wavefront that exist.  Lanes without a check start with `stale` in their
    landing registers.  Returns (bodies seen, {check: state records}, emu, generator)."""
    g = coopasm.generate_miller1(bits=bits)
    assert (g.S, g.SC) == (cg.LDS_WIDE_SLOTS, cg.LDS_WIDE_CONSTS) and g.n_line_steps == len(bits) + sum(bits) + 1
    p_limbs = [(cg.P >> (28 * i)) & 0xfffffff for i in range(NL)]
    subst = {"p%d" % i: v for i, v in enumerate(p_limbs)}
    subst.update({"pinv": (-pow(cg.P, -1, 1 << 28)) % (1 << 28), "act": "s[106:107]", "lines": "s[100:101]", "state": "s[110:111]", "stride": "s112"})
    emu = _WaveEmu(lanes=lanes, subst=subst)
    emu.geom = g
    emu.mem = _Recorder()
    act = sum(1 << c["lane"] for c in consts[:lanes] if c["active"])
    emu.s[100], emu.s[101], emu.s[106], emu.s[107], emu.s[110], emu.s[111], emu.s[112] = LINES_AT, 0, act & asmemu.M32, act >> 32, STATE_AT, 0, stride
    PS = g.PS

    def put(idx, limbs):
        for i in range(16):
            emu.lds[16 * idx + (i // 4) * PS * 16 + 4 * (i % 4)] = (limbs[i] if i < NL else 0) & asmemu.M32

    model_consts = cg.Emu().slot
    for c in range(g.SC):
        put(c, model_consts[cg.CONST_BASE + c])
    for r, row in enumerate(g.rows):
        for lig, ent in enumerate(row):
            for k in range(2):
                emu.lds[g.row_off[r] + 8 * lig + 4 * k] = ent[k] if ent else 0
    image = dict(emu.lds)
    for c in consts[:lanes]:
        for reg, val in ((g.vtab, c["vtab"]), (g.vgb, c["vgb"]), (g.F, g.flags[c["lig"]]), (g.vdst, c["vdst"]), (g.voff, c["voff"]),
                         (g.vland, c["vland"]), (g.vst, c["vst"])):
            emu.v.setdefault(reg, [None] * lanes)[c["lane"]] = val
        if not c["active"]:
            for r in range(8):
                emu.v.setdefault(g.L + r, [None] * lanes)[c["lane"]] = stale
    want_loads = {}
    for check, lines in lines_of.items():
        assert len(lines) == g.n_line_steps
        for s in range(g.n_line_steps):
            for c in range(6):
                limbs = cg.mont(lines[s][0][c])
                at = LINES_AT + ((s * 6 + c) * n_checks + check) * 64
                assert at + 64 <= LINES_AT + g.n_line_steps * stride
                for i in range(16):
                    emu.mem[at + 4 * i] = (limbs[i] if i < NL else 0) & asmemu.M32
                    want_loads[at + 4 * i] = 1
    emu.mem.armed = True
    seen = []

    def snap(e):
        def slot(grp, s):
            return [asmemu.s32(e.lds[16 * (g.SC + grp * g.SG + s) + (i // 4) * PS * 16 + 4 * (i % 4)]) for i in range(NL)]
        regs = [[asmemu.s32(e.v[g.A[0] + i][lane]) for i in range(NL)] for lane in range(lanes)]
        seen.append(([[slot(grp, s) for s in range(24)] for grp in range(lanes // 12)], regs))

    watch = {".Lm1_done_l_%=": snap, ".Lm1_done_s_%=": snap}
    watch.update(trace or {})
    emu.run(mutate(list(g.lines)) if mutate else g.lines, max_steps=50_000_000, watch=watch)
    emu.mem.armed = False
    assert emu.exec == (1 << lanes) - 1
    # global memory: every line record of every check of the wavefront read once, nothing else; the state records written, nothing else
    assert emu.mem.reads == want_loads
    states, want_stores = {}, set()
    for check in lines_of:
        recs = []
        for j in range(12):
            at = STATE_AT + ((j + st_off) * nc + check) * 64
            want_stores.update(range(at, at + 64, 4))
            recs.append([asmemu.s32(emu.mem[at + 4 * i]) for i in range(16)])
        states[check] = recs
    assert emu.mem.writes == want_stores
    # LDS: the constants and the operand table are what they were
    assert all(emu.lds[a] == v for a, v in image.items())
    return seen, states, emu, g


def _one_check_consts():
    """the twelve lanes of check 0 of a launch of one check - what the first three tests type out; test_lane_constants_* holds the
    program's answer to the same"""
    gb, PS = 16 * cg.LDS_WIDE_CONSTS, coopasm.generate_miller1(bits=ALL_BITS[:1]).PS
    return 6 * 64, [dict(lane=lig, grp=0, lig=lig, check=0, active=1, vgb=gb, vdst=gb + 16 * lig, vtab=8 * lig, voff=(lig >> 1) * 64 + (lig & 1) * 32,
                         vland=gb + 16 * (24 + (lig >> 1)) + (lig & 1) * 2 * PS * 16, vst=lig * 64) for lig in range(12)]


def test_lane_constants_of_the_kernel_header(plan_exe):
    """the stand-alone program's walk (the predicate at its edges, 32-bit offsets against 64-bit ones, under ASan and UBSan); its
    constants for the launch of one check are the ones the first tests of this file type out; kernel and host use the header"""
    out = subprocess.run([plan_exe], capture_output=True, text=True, timeout=600)
    _clean(out)
    assert re.search(r"miller1 plan_check ok: \d+ cases", out.stdout)
    stride, consts = _lane_constants(plan_exe, 0, 1, 1, 0)
    want_stride, want = _one_check_consts()
    assert stride == want_stride and [dict(c, active=1) for c in consts[:12]] == want and not any(c["active"] for c in consts[12:])
    for n, ok in ((164482, 1), (164483, 0)):
        out = subprocess.run([plan_exe, "0", str(n), str(n), "0"], capture_output=True, text=True, timeout=60)
        _clean(out)
        assert out.stdout.split("\n")[1] == "eligible %d" % ok
    with open(os.path.join(CSRC, "zkp_coop.hip")) as f:
        text = f.read()
    assert '#include "zkp_miller1_lanes.hpp"' in text and text.count("zkp::m1::eligible(") == 2 and "zkp::m1::lanes(lane, blockIdx.x" in text
    assert "* 6 * 64 * NLINES >> 32" not in text                      # the predicate is written once
    with open(os.path.join(CSRC, "zkp_miller1_lanes.hpp")) as f:
        text = f.read()
    assert "hip_runtime" not in text and "getenv" not in text


# ------------------------------------------------------------------------------------------------ full loop, one check
def _full_loop(lines):
    """all 62 iterations on twelve lanes, every body against the step model; returns (state records, trace of the iteration header)"""
    want, want_state = _model(lines, len(ALL_BITS))
    header, lo = [], []
    stride, consts = _one_check_consts()
    g0 = coopasm.generate_miller1(bits=ALL_BITS[:1])
    sIt = g0.sT
    trace = {".Lm1_bit_%=": lambda e: header.append((e.s[sIt], e.scc)), ".Lm1_lo_%=": lambda e: lo.append(e.s[sIt])}
    seen, states, emu, g = _run(ALL_BITS, 12, consts, stride, {0: lines}, 1, 1, trace=trace)
    assert g.lines == coopasm.generate_miller1().lines, "the block under test is the checked-in one"
    n_it, n_add = len(ALL_BITS), sum(ALL_BITS)
    assert (n_it, n_add, g.n_line_steps) == (62, 5, 68)
    assert len(seen) == len(want) == 62 + 5 + 62 + 1             # the watch labels: line products, second line products, squarings, the closing product
    for k, ((slots, regs), w) in enumerate(zip(seen, want)):
        for lane in range(12):
            assert regs[lane] == w[lane], (k, lane, "the fourteen result limbs")
            assert slots[0][lane] == w[lane], (k, lane, "result slot")
            assert slots[0][12 + lane] == w[12 + lane], (k, lane, "companion slot")
    state = states[0]
    for j in range(12):
        assert state[j][:NL] == want_state[j] and state[j][NL:] == [0, 0], (j, "state record")
    # the iteration header: every iteration reads its own add bit, iterations 32.. from the high mask word (taken: the branch around
    # the low word's s_bitcmp1); iteration 46 is the one addition iteration up there
    assert [it for it, _ in header] == list(range(62)) and [it for it, scc in header if scc] == [i for i, b in enumerate(ALL_BITS) if b]
    assert lo == list(range(32)) and ALL_BITS[46] and [i for i, b in enumerate(ALL_BITS) if b and i >= 32] == [46]
    assert emu.count["s_branch"] >= 30
    return state


def _seeded_pair(seed):
    rng = random.Random(seed)
    return m.g1_mul(m.G1_GEN, rng.randrange(2, 1 << 64)), m.g2_mul(m.G2_GEN, rng.randrange(2, 1 << 64))


@pytest.mark.parametrize("which", ("generator", "seeded"))
def test_whole_loop_gives_the_pairing_of_the_model(which):
    """62 iterations, 68 line steps.  Beside the step model at every body, independently of tools/coopgen.py: the twelve state records,
    out of Montgomery form, are the conjugated Miller value f^(p^6) - the loop parameter is negative - which
    bls12_381_model.final_exponentiation must raise to bls12_381_model.pairing(P, Q); conjugated back it gives the inverse."""
    p1, q = (m.G1_GEN, m.G2_GEN) if which == "generator" else _seeded_pair(0x3117)
    state = _full_loop(cg.model_lines([(p1, q)]))
    f = m.f12_from_flat_ints([cg.from_mont(state[j][:NL]) for j in range(12)])
    want = m.pairing(p1, q)
    assert m.final_exponentiation(f) == want and want != m.f12_one()
    assert m.f12_mul(m.final_exponentiation(m.f12_conj(f)), want) == m.f12_one()


def test_a_lost_or_short_wait_in_the_block_is_rejected():
    """what the counters are for: the block with one hand-counted wait weakened is refused by the rule that wait serves.
    lgkmcnt(9) -> (10) leaves a landing write queued when the next global_load takes its registers; the line product's wait without
    its vmcnt lets the landing writes read registers whose loads are in flight; a block cut off behind its entry ends with the first
    line records in flight"""
    stride, consts = _one_check_consts()
    lines = {0: _wave_lines(0)}

    def swap(old, new, count):
        def f(text):
            assert text.count(old) == count, (old, text.count(old))
            return [new if l == old else l for l in text]
        return f

    def go(mutate):
        return _run(ALL_BITS[:N_ITER], 12, consts, stride, lines, 1, 1, mutate=mutate)

    with pytest.raises(RuntimeError, match=r"global_load_dwordx4 v\[4:7\].*loads into v4, the data source of `ds_write_b128 v\d+, v\[4:7\]"):
        go(swap("s_waitcnt lgkmcnt(9)", "s_waitcnt lgkmcnt(10)", 1))
    with pytest.raises(RuntimeError, match=r"ds_write_b128 v\d+, v\[0:3\]` touches v0, the destination of `global_load_dwordx4 v\[0:3\]"):
        go(swap("s_waitcnt vmcnt(0) lgkmcnt(0)", "s_waitcnt lgkmcnt(0)", 2))
    with pytest.raises(RuntimeError, match=r"the block ends with `global_load_dwordx4 v\[0:3\].*still in flight \(v0\)"):
        go(lambda text: text[:text.index(".Lm1_iter_%=:")])


# ------------------------------------------------------------------------------------------------ the whole wavefront
WAVE_CASES = ((0, 1, 1, 0), (0, 3, 3, 0), (0, 5, 7, 0), (1, 8, 11, 2), (2, 11, 320, 0))      # (block, n_checks, nc, st_off)
STALE = (0x7fffffff, 0x80000000)
_one_check_states = {}


def _wave_lines(check):
    """a different pair for every check of a launch"""
    p1, q = (m.G1_GEN, m.G2_GEN) if check == 0 else _seeded_pair(0x5EED00 + check)
    n = N_ITER + sum(ALL_BITS[:N_ITER]) + 1
    return cg.model_lines([(p1, q)])[:n]


def _one_check_state(check):
    """the state records of the check's pair run alone: one check, twelve lanes (the run the first test holds to the step model)"""
    if check not in _one_check_states:
        stride, consts = _one_check_consts()
        _, states, _, _ = _run(ALL_BITS[:N_ITER], 12, consts, stride, {0: _wave_lines(check)}, 1, 1)
        _one_check_states[check] = states[0]
    return _one_check_states[check]


@pytest.mark.parametrize("block,n_checks,nc,st_off", WAVE_CASES)
def test_whole_wavefront(plan_exe, block, n_checks, nc, st_off):
    """sixty lanes, three iterations, the lane constants from the kernel's header: the only block with one and with three checks, a
    full block in a wider state buffer, the partial second block of a launch with an element offset, the last block (one check) of
    a launch that writes a 320-check state buffer.  Lanes of groups without a check hold stale landing registers (both extremes).
    _run asserts: the global words read are the six line records of every check and line step, once each, all inside the line buffer;
    the words written are the twelve state records of every check at ((j + st_off) * nc + check) * 64; constants and operand table
    are unchanged; every LDS write stays in the writer's group (_WaveEmu).  Here: each check's records are those of its pair run alone."""
    stride, consts = _lane_constants(plan_exe, block, n_checks, nc, st_off)
    checks = [c for c in range(5 * block, 5 * block + 5) if c < n_checks]
    assert checks and sorted({c["check"] for c in consts if c["active"]}) == checks
    lines_of = {c: _wave_lines(c) for c in checks}
    for stale in STALE if len(checks) < 5 else (None,):
        seen, states, emu, g = _run(ALL_BITS[:N_ITER], 60, consts, stride, lines_of, n_checks, nc, st_off, stale=stale)
        assert len(seen) == N_ITER + sum(ALL_BITS[:N_ITER]) + N_ITER + 1
        for c in checks:
            assert states[c] == _one_check_state(c), (c, stale)
        assert len(emu.mem.writes) == 12 * 16 * len(checks) and len(emu.mem.reads) == g.n_line_steps * 6 * 16 * len(checks)


# ------------------------------------------------------------------------------------------------ adversarial line streams
SEARCH_SEED, SEARCH_N = 0x51EA0000, 200
SEARCH_BEST = (161, 840897539526885376)        # candidate, its largest |reduction column| (59.5 bits)


def _pool():
    import adversarial as adv
    vals = [o.v for o in adv.pool()]
    assert {0, 1, cg.P - 1, (cg.P - 1) // 2} <= set(vals)
    return vals


def _drawn_stream(seed):
    rng, vals = random.Random(seed), _pool()
    return [[[rng.choice(vals) for _ in range(6)]] for _ in range(len(ALL_BITS) + sum(ALL_BITS) + 1)]


def _searched_stream():
    """the candidate, of SEARCH_N drawn streams, whose first three iterations drive the step model's reduction columns highest"""
    prog, best = _short_program(N_ITER), (0, None)
    try:
        for k in range(SEARCH_N):
            cg.STATS = {}
            cg.Emu(lines=_drawn_stream(SEARCH_SEED + k)).run(prog)
            best = max(best, (cg.STATS["red_col"], k))
    finally:
        cg.STATS = None
    assert (best[1], best[0]) == SEARCH_BEST
    return _drawn_stream(SEARCH_SEED + best[1])


@pytest.mark.parametrize("stream", ("all_p_minus_1", "drawn", "searched"))
def test_whole_loop_on_adversarial_line_streams(stream):
    """the kernel is data-oblivious: any six field values are a line step.  Streams from tests/adversarial.py's pool (0, 1, p - 1,
    (p - 1) / 2, the limb-boundary values of every geometry, their Montgomery pre-images) through the whole loop on twelve lanes,
    every body against the step model - whose own asserts (accumulation columns below 2^62, reduction columns and carries inside an
    int64, limbs inside an int32) are the overflow check: the block computes the same integers.
    all_p_minus_1: every coefficient p - 1.  drawn: seed 0xAD51.  searched: of 200 streams drawn with seeds 0x51EA0000 + k, the one
    whose first three iterations give the largest |reduction column| - k = 161, 840897539526885376 (2^59.5; the int64 limit is 2^63)."""
    n = len(ALL_BITS) + sum(ALL_BITS) + 1
    lines = {"all_p_minus_1": lambda: [[[cg.P - 1] * 6] for _ in range(n)], "drawn": lambda: _drawn_stream(0xAD51), "searched": _searched_stream}[stream]()
    _full_loop(lines)
