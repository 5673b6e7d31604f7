#!/usr/bin/env python3
"""A CPU model of the gfx950 instruction subset that tools/coopasm.py emits - the gate for the generated inline-asm blocks.

It executes the text of a generated block (scalar branches and loops included) on a group of lanes: 32-bit VGPRs per lane, SGPRs,
EXEC, an LDS byte image, DPP quad permutations.  Two things a GPU run would only show as wrong numbers are errors here:
a DPP read from a lane that EXEC has switched off, and a read of a register nothing has written.

    emu = Emu(lanes=4, subst={"p0": ..., "pinv": ...})
    emu.v[6][lane] = ...          # operands
    emu.run(lines)
    emu.v[6][lane]                # results (uint32; s32() for the signed value)

tests/test_coopasm.py runs the k_ksq body against tools/coopgen.py's limb-exact model of a compressed squaring.

Two more checks are on by default (Emu(counters=True, wait_states=True)); tests/test_asmemu_cpu.py holds one accepted and one
rejected snippet for every rule.  Both follow the ONE path the emulator executes; the state is reset at the start of run().

Memory counters.  Every global_load_* / global_store_* enters the VM queue, every ds_read_* / ds_write_* (and s_load_*) the LGKM
queue.  `s_waitcnt vmcnt(N)` / `lgkmcnt(N)` retires all but the youngest N entries of its queue, oldest first (gfx9 returns vector
memory and LDS accesses in order); a count that the instruction does not name leaves its queue alone; vmcnt > 63 or lgkmcnt > 15 cannot
be encoded and is an error.  Once a block has issued a scalar memory load a nonzero lgkmcnt retires nothing (scalar loads return out
of order: only lgkmcnt(0) says anything).  Errors, each naming the instruction and the register:
  (a) an instruction reads or overwrites a VGPR that is the destination of a load still in its queue;
  (b) a load is given a destination that is the data source of an LDS write or a global store still in its queue.  This is the
      CONSERVATIVE rule (the hardware may well have read the data by then); no checked-in block needed it narrowed;
  (c) run() reaches the end of the text with a load still queued: behind the block the compiler may reuse any clobbered register.

Wait states the hardware does not insert.  One state per instruction issued in between, `s_nop N` counts N + 1:
  * a VALU write of a VGPR -> a DPP instruction that reads it (any of its vector sources): 2 states;
  * a VALU write of an SGPR (v_readfirstlane_b32, the carry-out of v_mad_*64) -> a vector memory instruction that uses it as
    saddr: 5 states.  The instruction-set manual's table of required wait states has "VALU writes SGPR -> VMEM reads that SGPR: 5"
    and NO row for an SALU write (the scalar unit's writes are interlocked); LLVM's GCNHazardRecognizer::checkVMEMHazards pads the
    same case only.  A rule that also covered SALU writes was tried first: k_coop's MULACC block trips it in every term (s_addc_u32
    of the table pointer, then the global_load that uses it, nothing in between) and has been byte-exact on the GPU since it was
    written - DESIGN.md section 3 records the finding;
  * added from the same source (a store of more than 64 bits -> a write of its data registers: 2 states, "s_nop 1"), because the
    generators emit global_store_dwordx4 and VALU writes of the stored registers: an overwrite of a data register of a
    global_store_dwordx3/x4 that is still in the VM queue needs 2 states behind the store.
What the emulator still cannot see: latency, LDS bank conflicts, instruction-cache effects - anything that depends on time.
"""
import functools
import re

M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def s24(x):
    x &= 0xffffff
    return x - (1 << 24) if x >> 23 else x


@functools.lru_cache(maxsize=None)
def _regs(text, kind):
    out = set()
    for m in re.finditer(r"(?<![\w\[:])%s(?:(\d+)|\[(\d+):(\d+)\])" % kind, text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return frozenset(out)


@functools.lru_cache(maxsize=None)
def _operand(op):
    """("v" | "s", first register, number of registers of a range or None) or ("i", value, None)"""
    op = op.strip()
    m = re.fullmatch(r"([vs])\[(\d+):(\d+)\]", op)
    if m:
        return m.group(1), int(m.group(2)), int(m.group(3)) - int(m.group(2)) + 1
    m = re.fullmatch(r"([vs])(\d+)", op)
    if m:
        return m.group(1), int(m.group(2)), None
    return "i", int(op, 0), None


class Emu:
    DPP_STATES, SADDR_STATES, STORE_DATA_STATES = 2, 5, 2

    def __init__(self, lanes=4, subst=None, strict=True, counters=True, wait_states=True):
        self.n = lanes
        self.v = {}                 # register number -> [value per lane]
        self.s = {}
        self.exec = (1 << lanes) - 1
        self.lds = {}               # byte address -> dword (addresses are multiples of 4)
        self.mem = {}               # global memory: byte address -> dword
        self.scc = 0
        self.vcc = 0
        self.subst = dict(subst or {})
        self.strict = strict
        self.count = {}
        self.counters = counters
        self.wait_states = wait_states
        self._reset_hazards()

    # ---- memory counters and wait states
    def _reset_hazards(self):
        self.vmq, self.lgkmq = [], []      # entries: (kind, registers, instruction text[, clock]); kind "load" / "store" / "sload"
        self.smem_seen = False
        self.clock = 0                     # wait states issued so far
        self.valu_vgpr, self.valu_sgpr = {}, {}      # register -> clock of the VALU instruction that wrote it last

    @staticmethod
    def _regs(text, kind):
        """the registers of one kind ("v" / "s") that an operand text names"""
        return _regs(text, kind)

    def _waitcnt(self, line):
        rest, seen = line.split(None, 1)[1] if " " in line else "", False
        for name, q, top in (("vmcnt", self.vmq, 63), ("lgkmcnt", self.lgkmq, 15)):
            m = re.search(name + r"\((\d+)\)", rest)
            if not m:
                continue
            seen, n = True, int(m.group(1))
            if n > top:
                raise RuntimeError("%s(%d) cannot be encoded (at most %d): %s" % (name, n, top, line))
            if name == "lgkmcnt" and n and self.smem_seen:
                continue                   # scalar loads return out of order: a nonzero count proves nothing
            del q[:max(len(q) - n, 0)]
        if not seen:
            raise NotImplementedError("s_waitcnt without vmcnt() / lgkmcnt(): " + line)

    def _hazards(self, op, args, line):
        """called before `line` executes: the rules of the module docstring"""
        text = ", ".join(args)
        vregs = self._regs(text, "v")
        is_vm, is_ds, is_smem = op.startswith("global_"), op.startswith("ds_"), op.startswith("s_load") or op.startswith("s_buffer_load")
        is_valu = op.startswith("v_")
        store = "store" in op or "write" in op
        if self.counters:
            for q in (self.vmq, self.lgkmq):
                for ent in q:
                    if ent[0] == "load" and vregs & ent[1]:
                        raise RuntimeError("`%s` touches v%d, the destination of `%s`, which is still in flight (no s_waitcnt has retired it)"
                                           % (line, min(vregs & ent[1]), ent[2]))
            if (is_vm or is_ds) and not store:
                dst = self._regs(args[0], "v")
                for q in (self.vmq, self.lgkmq):
                    for ent in q:
                        if ent[0] == "store" and dst & ent[1]:
                            raise RuntimeError("`%s` loads into v%d, the data source of `%s`, which is still in its queue"
                                               % (line, min(dst & ent[1]), ent[2]))
        if self.wait_states:
            if op.endswith("_dpp"):
                for r in sorted(self._regs(", ".join(args[1:]), "v")):
                    if r in self.valu_vgpr and self.clock - self.valu_vgpr[r] - 1 < self.DPP_STATES:
                        raise RuntimeError("`%s` reads v%d by DPP %d wait state(s) behind the VALU write of it: %d are required"
                                           % (line, r, self.clock - self.valu_vgpr[r] - 1, self.DPP_STATES))
            if is_vm:
                for r in sorted(self._regs(args[2], "s")):
                    if r in self.valu_sgpr and self.clock - self.valu_sgpr[r] - 1 < self.SADDR_STATES:
                        raise RuntimeError("`%s` takes its address from s%d %d wait state(s) behind the VALU write of it: %d are required"
                                           % (line, r, self.clock - self.valu_sgpr[r] - 1, self.SADDR_STATES))
            written = set()
            if is_valu:
                written = self._valu_dst(op, args)
            elif (is_vm or is_ds) and not store:
                written = self._regs(args[0], "v")
            for ent in self.vmq:
                if ent[0] == "store" and len(ent[1]) > 2 and written & ent[1] and self.clock - ent[3] - 1 < self.STORE_DATA_STATES:
                    raise RuntimeError("`%s` overwrites v%d %d wait state(s) behind `%s`, which stores it: %d are required"
                                       % (line, min(written & ent[1]), self.clock - ent[3] - 1, ent[2], self.STORE_DATA_STATES))
        # ---- what the instruction leaves behind
        if is_vm or is_ds:
            q = self.vmq if is_vm else self.lgkmq
            q.append(("store", self._regs(args[1], "v"), line, self.clock) if store else ("load", self._regs(args[0], "v"), line, self.clock))
        if is_smem:
            self.smem_seen = True
            self.lgkmq.append(("sload", set(), line, self.clock))
        if is_valu:
            for r in self._valu_dst(op, args):
                self.valu_vgpr[r] = self.clock
            sdst = args[0] if op.startswith("v_readfirstlane") else args[1] if op.startswith(("v_mad_i64", "v_mad_u64")) else ""
            for r in self._regs(sdst, "s"):
                self.valu_sgpr[r] = self.clock
        elif op.startswith("s_") and args:
            for r in self._regs(args[0], "s"):
                self.valu_sgpr.pop(r, None)         # an SALU write is interlocked

    def _valu_dst(self, op, args):
        if op.startswith("v_cmp") or op.startswith("v_readfirstlane"):
            return set()
        if op.startswith("v_swap"):
            return self._regs(args[0], "v") | self._regs(args[1], "v")
        return self._regs(args[0], "v")

    def _at_end(self):
        if self.counters:
            for q in (self.vmq, self.lgkmq):
                for ent in q:
                    if ent[0] != "store":
                        raise RuntimeError("the block ends with `%s` still in flight%s: the code behind it may reuse the register"
                                           % (ent[2], " (v%d)" % min(ent[1]) if ent[1] else ""))

    # ---- operands
    def _sub(self, text):
        return re.sub(r"%\[(\w+)\]", lambda m: str(self.subst[m.group(1)]), text)

    def rd(self, op, lane, width=1):
        """value of a source operand for one lane (width = number of dwords)"""
        kind, lo, n = _operand(op)
        if kind == "v":
            if n is None:
                assert width == 1, op
                return self._rv(lo, lane)
            assert n == width, op
            return sum(self._rv(lo + k, lane) << (32 * k) for k in range(width))
        if kind == "s":
            if n is None:
                v = self.s[lo]
                return v if width == 1 else s32(v) & M64      # a 32-bit scalar source of a 64-bit operand is sign-extended
            return sum(self.s[lo + k] << (32 * k) for k in range(n))
        return lo & (M32 if width == 1 else M64)

    def _rv(self, r, lane):
        if r not in self.v or self.v[r][lane] is None:
            if self.strict:
                raise RuntimeError("read of unwritten v%d (lane %d)" % (r, lane))
            return 0
        return self.v[r][lane]

    def wr(self, op, lane, val, width=1):
        kind, lo, n = _operand(op)
        assert kind == "v", op
        if n is None:
            assert width == 1, op
            self.v.setdefault(lo, [None] * self.n)[lane] = val & M32
            return
        assert n == width and lo % 2 == 0, "misaligned or mis-sized tuple " + op
        for k in range(width):
            self.v.setdefault(lo + k, [None] * self.n)[lane] = (val >> (32 * k)) & M32

    # ---- execution
    def run(self, lines, max_steps=10_000_000, watch=None):
        """watch: {label: function(emu)} - called whenever execution passes the label (looping code: once per pass)"""
        prog = [self._sub(l).strip() for l in lines]
        prog = [l for l in prog if l]
        labels = {l[:-1]: i for i, l in enumerate(prog) if l.endswith(":")}
        self._reset_hazards()
        pc, n = 0, 0
        while pc < len(prog):
            line = prog[pc]
            pc += 1
            if line.endswith(":"):
                if watch and line[:-1] in watch:
                    watch[line[:-1]](self)
                continue
            n += 1
            assert n < max_steps, "runaway loop"
            op = line.split(None, 1)[0]
            if op in ("s_branch", "s_cbranch_scc0", "s_cbranch_scc1"):
                self.count[op] = self.count.get(op, 0) + 1
                self.clock += 1
                target = line.split(None, 1)[1].strip()
                if op == "s_branch" or (op == "s_cbranch_scc1") == bool(self.scc):
                    pc = labels[target]
                continue
            self.step(line)
        self._at_end()
        return self

    def step(self, line):
        mods, raw = {}, line
        m = re.search(r"quad_perm:\[(\d),(\d),(\d),(\d)\]", line)
        if m:
            mods["qp"] = [int(x) for x in m.groups()]
            line = line[:m.start()] + line[m.end():]
        for key in ("row_mask", "bank_mask", "offset"):
            m = re.search(key + r":(0x[0-9a-fA-F]+|\d+)", line)
            if m:
                mods[key] = int(m.group(1), 0)
                line = line[:m.start()] + line[m.end():]
        parts = line.split(None, 1)
        op = parts[0]
        args = [a.strip() for a in self._split(parts[1])] if len(parts) > 1 else []
        self.count[op] = self.count.get(op, 0) + 1
        dpp = op.endswith("_dpp")
        if dpp:
            op = op[:-4]
            assert mods.get("row_mask", 0xf) == 0xf and mods.get("bank_mask", 0xf) == 0xf and "qp" in mods
            if op in ("v_subrev_u32",):
                # measured on gfx950 (tools/dbg/dpp_probe.hip): v_subrev_u32_dpp d, x, zero returns 0 - x of the lane ITSELF
                raise NotImplementedError("v_subrev_u32_dpp does not permute its subtrahend on gfx950")
        fn = getattr(self, "op_" + op, None)
        if fn is None:
            raise NotImplementedError(op)
        if op == "s_waitcnt" and self.counters:
            self._waitcnt(raw)
        self._hazards(parts[0], args, raw)
        self.clock += 1 + (int(args[0], 0) if op == "s_nop" else 0)
        if op.startswith("s_") or op.startswith("ds_") or op.startswith("global_"):
            fn(args, mods)
            return
        for lane in range(self.n):
            if not (self.exec >> lane) & 1:
                continue
            src_lane = lane
            if dpp:
                src_lane = (lane & ~3) | mods["qp"][lane & 3]
                if not (self.exec >> src_lane) & 1:
                    raise RuntimeError("DPP read from lane %d, which EXEC has switched off: %s" % (src_lane, line))
            fn(args, lane, src_lane)

    @staticmethod
    def _split(s):
        out, depth, cur = [], 0, ""
        for ch in s:
            if ch == "[":
                depth += 1
            if ch == "]":
                depth -= 1
            if ch == "," and depth == 0:
                out.append(cur)
                cur = ""
            else:
                cur += ch
        if cur.strip():
            out.append(cur)
        return out

    # ---- scalar / LDS
    def op_s_nop(self, a, m):
        pass

    def op_s_waitcnt(self, a, m):
        pass                    # (step() has retired the queues: _waitcnt)

    def op_s_load_dword(self, a, m, n=1):        # sdst, sbase, offset
        addr = self.rd(a[1], 0) + int(a[2], 0)
        lo = int(re.match(r"s\[?(\d+)", a[0].strip()).group(1))
        for k in range(n):
            if addr + 4 * k not in self.mem:
                raise RuntimeError("scalar read of unwritten address 0x%x" % (addr + 4 * k))
            self.s[lo + k] = self.mem[addr + 4 * k]

    def op_s_load_dwordx2(self, a, m):
        self.op_s_load_dword(a, m, 2)

    def op_v_readfirstlane_b32(self, a, l, sl):
        if l == min(i for i in range(self.n) if (self.exec >> i) & 1):
            self.s[int(a[0].strip()[1:])] = self.rd(a[1], l)

    def op_s_setprio(self, a, m):
        pass

    def op_s_mov_b32(self, a, m):
        self.s[int(a[0][1:])] = int(a[1], 0) & M32 if not a[1].startswith("s") else self.s[int(a[1][1:])]

    def op_s_mov_b64(self, a, m):
        if a[0] == "vcc":
            self.vcc = self.rd(a[1], 0)
            return
        if a[0] == "exec":
            self.exec = self.rd(a[1], 0) & ((1 << self.n) - 1) if a[1] != "-1" else (1 << self.n) - 1
            return
        lo = int(re.match(r"s\[(\d+):", a[0]).group(1))
        val = ((1 << 64) - 1 if self.exec == (1 << self.n) - 1 else self.exec) if a[1] == "exec" else self.rd(a[1], 0)
        self.s[lo], self.s[lo + 1] = val & M32, (val >> 32) & M32

    def _rd64(self, x):
        x = x.strip()
        if x == "vcc":
            return self.vcc
        if x == "exec":
            return self.exec
        return self.rd(x, 0)

    def op_s_and_b64(self, a, m):
        val = self._rd64(a[1]) & self._rd64(a[2])
        d = a[0].strip()
        if d == "vcc":
            self.vcc = val
        elif d == "exec":
            self.exec = val & ((1 << self.n) - 1)
        else:
            lo = int(re.match(r"s\[(\d+):", d).group(1))
            self.s[lo], self.s[lo + 1] = val & M32, (val >> 32) & M32
        self.scc = int(val != 0)

    def op_s_cmp_lg_u32(self, a, m):
        self.scc = int(self._sr(a[0]) != self._sr(a[1]))

    def _sr(self, x):
        x = x.strip()
        return self.s[int(x[1:])] if re.fullmatch(r"s\d+", x) else int(x, 0) & M32

    def _sw(self, x, v):
        self.s[int(x.strip()[1:])] = v & M32

    def op_s_lshr_b32(self, a, m):
        self._sw(a[0], self._sr(a[1]) >> (self._sr(a[2]) & 31))
        self.scc = int(self._sr(a[0]) != 0)

    def op_s_lshl_b32(self, a, m):
        self._sw(a[0], self._sr(a[1]) << (self._sr(a[2]) & 31))
        self.scc = int(self._sr(a[0]) != 0)

    def op_s_and_b32(self, a, m):
        self._sw(a[0], self._sr(a[1]) & self._sr(a[2]))
        self.scc = int(self._sr(a[0]) != 0)

    def op_s_add_u32(self, a, m):
        v = self._sr(a[1]) + self._sr(a[2])
        self._sw(a[0], v)
        self.scc = v >> 32

    def op_s_addc_u32(self, a, m):
        v = self._sr(a[1]) + self._sr(a[2]) + self.scc
        self._sw(a[0], v)
        self.scc = v >> 32

    def op_s_mul_i32(self, a, m):
        self._sw(a[0], s32(self._sr(a[1])) * s32(self._sr(a[2])))

    def op_s_mul_hi_u32(self, a, m):
        self._sw(a[0], (self._sr(a[1]) * self._sr(a[2])) >> 32)

    def op_s_cmp_ge_u32(self, a, m):
        self.scc = int(self._sr(a[0]) >= self._sr(a[1]))

    def op_s_cmp_lt_u32(self, a, m):
        self.scc = int(self._sr(a[0]) < self._sr(a[1]))

    def op_s_cmp_eq_u32(self, a, m):
        self.scc = int(self._sr(a[0]) == self._sr(a[1]))

    def op_s_bitcmp1_b32(self, a, m):
        self.scc = (self._sr(a[0]) >> (self._sr(a[1]) & 31)) & 1

    def _gload(self, a, m, n):
        base = self.rd(a[2], 0) if a[2].strip() != "off" else 0
        for lane in range(self.n):
            if (self.exec >> lane) & 1:
                addr = base + self.rd(a[1], lane) + m.get("offset", 0)
                assert addr % 4 == 0
                for k in range(n):
                    if addr + 4 * k not in self.mem:
                        raise RuntimeError("global read of unwritten address 0x%x" % (addr + 4 * k))
                    self.v.setdefault(self._vbase(a[0]) + k, [None] * self.n)[lane] = self.mem[addr + 4 * k]

    @staticmethod
    def _vbase(op):
        mm = re.fullmatch(r"v\[(\d+):(\d+)\]", op.strip())
        return int(mm.group(1)) if mm else int(op.strip()[1:])

    def op_global_store_dwordx4(self, a, m):     # voffset, vdata[4], saddr
        base = self.rd(a[2], 0)
        for lane in range(self.n):
            if (self.exec >> lane) & 1:
                addr = base + self.rd(a[0], lane) + m.get("offset", 0)
                assert addr % 16 == 0
                val = self.rd(a[1], lane, 4)
                for k in range(4):
                    self.mem[addr + 4 * k] = (val >> (32 * k)) & M32

    def op_global_load_dwordx4(self, a, m):
        self._gload(a, m, 4)

    def op_global_load_dwordx3(self, a, m):
        self._gload(a, m, 3)

    def op_global_load_dwordx2(self, a, m):
        self._gload(a, m, 2)

    def op_ds_read_b64(self, a, m):
        off = m.get("offset", 0)
        for lane in range(self.n):
            if (self.exec >> lane) & 1:
                addr = self.rd(a[1], lane) + off
                assert addr % 8 == 0
                for k in range(2):
                    if addr + 4 * k not in self.lds:
                        raise RuntimeError("LDS read of unwritten address %d" % (addr + 4 * k))
                self.wr(a[0], lane, sum(self.lds[addr + 4 * k] << (32 * k) for k in range(2)), 2)

    def op_ds_read_b128(self, a, m):
        off = m.get("offset", 0)
        for lane in range(self.n):
            if (self.exec >> lane) & 1:
                addr = self.rd(a[1], lane) + off
                assert addr % 16 == 0
                for k in range(4):
                    if addr + 4 * k not in self.lds:
                        raise RuntimeError("LDS read of unwritten address %d" % (addr + 4 * k))
                self.wr(a[0], lane, sum(self.lds[addr + 4 * k] << (32 * k) for k in range(4)), 4)

    def op_ds_write_b64(self, a, m):
        off = m.get("offset", 0)
        for lane in range(self.n):
            if (self.exec >> lane) & 1:
                addr = self.rd(a[0], lane) + off
                assert addr % 8 == 0
                val = self.rd(a[1], lane, 2)
                for k in range(2):
                    self.lds[addr + 4 * k] = (val >> (32 * k)) & M32

    def op_ds_write_b128(self, a, m):
        off = m.get("offset", 0)
        for lane in range(self.n):
            if (self.exec >> lane) & 1:
                addr = self.rd(a[0], lane) + off
                assert addr % 16 == 0
                val = self.rd(a[1], lane, 4)
                for k in range(4):
                    self.lds[addr + 4 * k] = (val >> (32 * k)) & M32

    # ---- vector
    def op_v_cmp_ne_u32_e32(self, a, l, sl):     # vcc[lane] = src0 != src1 (lanes EXEC has switched off keep their bit clear)
        assert a[0].strip() == "vcc"
        if l == min(i for i in range(self.n) if (self.exec >> i) & 1):
            self.vcc = 0
        if (self.rd(a[1], l) & M32) != (self.rd(a[2], l) & M32):
            self.vcc |= 1 << l

    def op_v_swap_b32(self, a, l, sl):
        x, y = self.rd(a[0], l), self.rd(a[1], l)
        self.wr(a[0], l, y)
        self.wr(a[1], l, x)

    def op_v_mov_b32(self, a, l, sl):
        self.wr(a[0], l, self.rd(a[1], sl))

    def op_v_cndmask_b32(self, a, l, sl):        # d = vcc[lane] ? src1 : src0
        assert a[3].strip() == "vcc"
        self.wr(a[0], l, self.rd(a[2], l) if (self.vcc >> l) & 1 else self.rd(a[1], l))

    def op_v_add_u32(self, a, l, sl):
        self.wr(a[0], l, self.rd(a[1], sl) + self.rd(a[2], l))

    def op_v_sub_u32(self, a, l, sl):
        self.wr(a[0], l, self.rd(a[1], sl) - self.rd(a[2], l))

    def op_v_subrev_u32(self, a, l, sl):
        self.wr(a[0], l, self.rd(a[2], l) - self.rd(a[1], sl))

    def op_v_and_b32(self, a, l, sl):
        self.wr(a[0], l, self.rd(a[1], sl) & self.rd(a[2], l))

    def op_v_xad_u32(self, a, l, sl):
        self.wr(a[0], l, (self.rd(a[1], l) ^ self.rd(a[2], l)) + self.rd(a[3], l))

    def op_v_lshrrev_b32(self, a, l, sl):
        self.wr(a[0], l, self.rd(a[2], l) >> (self.rd(a[1], l) & 31))

    def op_v_bfe_u32(self, a, l, sl):
        x, off, w = self.rd(a[1], l), self.rd(a[2], l) & 31, self.rd(a[3], l) & 31
        self.wr(a[0], l, (x >> off) & ((1 << w) - 1))

    def op_v_lshlrev_b32(self, a, l, sl):
        self.wr(a[0], l, self.rd(a[2], l) << (self.rd(a[1], l) & 31))

    def op_v_ashrrev_i32(self, a, l, sl):
        self.wr(a[0], l, s32(self.rd(a[2], l)) >> (self.rd(a[1], l) & 31))

    def op_v_lshl_add_u32(self, a, l, sl):
        self.wr(a[0], l, (self.rd(a[1], l) << (self.rd(a[2], l) & 31)) + self.rd(a[3], l))

    def op_v_bfe_i32(self, a, l, sl):
        x, off, w = self.rd(a[1], l), self.rd(a[2], l) & 31, self.rd(a[3], l) & 31
        f = (x >> off) & ((1 << w) - 1)
        self.wr(a[0], l, f - (1 << w) if w and (f >> (w - 1)) else f)

    def op_v_mul_lo_u32(self, a, l, sl):
        self.wr(a[0], l, self.rd(a[1], l) * self.rd(a[2], l))

    def op_v_mul_i32_i24(self, a, l, sl):
        self.wr(a[0], l, s24(self.rd(a[1], l)) * s24(self.rd(a[2], l)))

    def op_v_mad_i32_i24(self, a, l, sl):
        self.wr(a[0], l, s24(self.rd(a[1], l)) * s24(self.rd(a[2], l)) + self.rd(a[3], l))

    def op_v_mad_i64_i32(self, a, l, sl):      # vdst, sdst (carry out, ignored), a, b, c
        self.wr(a[0], l, s32(self.rd(a[2], l)) * s32(self.rd(a[3], l)) + self.rd(a[4], l, 2), 2)

    def op_v_mad_u64_u32(self, a, l, sl):
        self.wr(a[0], l, self.rd(a[2], l) * self.rd(a[3], l) + self.rd(a[4], l, 2), 2)

    def op_v_lshl_add_u64(self, a, l, sl):
        self.wr(a[0], l, (self.rd(a[1], l, 2) << (self.rd(a[2], l) & 63)) + self.rd(a[3], l, 2), 2)

    def op_v_ashrrev_i64(self, a, l, sl):
        self.wr(a[0], l, s64(self.rd(a[2], l, 2)) >> (self.rd(a[1], l) & 63), 2)

    def op_v_mbcnt_lo_u32_b32(self, a, l, sl):
        self.wr(a[0], l, min(l, 32) + self.rd(a[2], l))      # mask -1: the number of lower lanes among lanes 0..31

    def op_v_mbcnt_hi_u32_b32(self, a, l, sl):
        self.wr(a[0], l, max(l - 32, 0) + self.rd(a[2], l))
