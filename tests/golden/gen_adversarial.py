#!/usr/bin/env python3
"""Search the bit-accurate CPU models for operands that drive their internal quantities to the limits, and write the best ones to
tests/golden/adversarial_operands.json.  A seeded hill-climb: start from the pool records of tests/adversarial.py, mutate single
coefficients / limbs / bits, keep improvements; one internal quantity (target) at a time.

  tools/coopgen.py (the 28-bit cooperative core), per program: widest accumulation column (max_col), widest column inside the
      reduction (red_col), largest |q| of vred / the MULACC epilogue / sq_combine (q_vred, q_epi, q_sq), reduced value closest to
      the 0.51 p bound (reduced), canonical_from_reduced input closest to 2p / -p (canon_hi, canon_lo), largest limb entering
      weak_norm (wn_limb)
  tools/safegcd_model.py (the division-step inversion, packed formulation): most batches until g == 0 (batches), d / e closest to
      p / -2p (de_hi, de_lo), largest matrix entry of a run of ten steps and of a batch (run_max, entry_max)

The maxima are LOWER bounds on the true worst case, not proofs.  Deterministic: SplitMix64 with the seed below.
Run: python3 tests/golden/gen_adversarial.py"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "tools")]
import adversarial as adv  # noqa: E402
import bls12_381_model as m  # noqa: E402
import coopgen as cg  # noqa: E402
import safegcd_model as sgm  # noqa: E402

P = m.P
SEED = 0x5EA2C4
EVALS_PER_CLIMB = 24          # emulator evaluations per (program, target) beyond the pool records every program starts from
EVALS_DIVSTEP = 400           # inversions per division-step target beyond the pool
EMU_TARGETS = ("max_col", "red_col", "q_vred", "q_epi", "q_sq", "reduced", "canon_hi", "canon_lo", "wn_limb")
SG_TARGETS = ("batches", "de_hi", "de_lo", "run_max", "entry_max")
DESCENT_SWEEPS = 2            # coordinate-descent sweeps over the coefficients with the extreme stored digit patterns (max_col, red_col)
KSQ_NSQ, KSQ_MASK = 3, 0b101
# longer compressed squaring runs (squarings, snapshot mask) and the exceptional decompression branches: replayed on a thinner set of
# pool records, not climbed (a 63-squaring run costs twenty times the short one)
KSQ_LONG = {"ksq:63": (63, cg.KSQ_MASK), "ksq:48": (48, 1 << 47 | 1 << 1), "ksq:17": (17, 1 << 16 | 1 << 15 | 1), "ksq:1": (1, 1)}
KDEC_BRANCH = {"kdec": 0, "kdec:z2=0": 1, "kdec:z2=z3=0": 2}


def programs():
    """name -> (width of a, width of b or 0)"""
    out = {}
    wid = {"fp2": 2, "fp6": 6, "fp1": 12, "cyc": 12}
    for op in cg.TOWER_OPS:
        out["tower:" + op] = (wid[op[:3]], {"fp2_mul": 2, "fp6_mul": 6, "fp12_mul": 12, "fp12_014": 6}.get(op, 0))
    for op in cg.TOWER_OPS2:
        out["tower2:" + op] = (wid[op[:3]], {"fp2_mulfp": 1, "fp6_by1": 2, "fp6_by01": 4}.get(op, 0))
    for w in ("fp2", "fp6", "fp12"):
        out["inv:" + w] = (wid[w[:3]], 0)
    out["ksq"] = (12, 0)
    for k in KSQ_LONG:
        out[k] = (12, 0)
    for k in KDEC_BRANCH:
        out[k] = (12, 0)
    return out


def extremes():
    """the R = 2^392 pre-images whose stored representative has every digit below the top at +(2^27 - 1) or at -2^27: what the
    coordinate descent puts into one coefficient at a time"""
    ops = [o for o in adv.limb_boundaries() if "balanced-digits" in o.name]
    return [o.v for o in adv.preimages(ops, adv.R28, "pre28")]


def ksq_params(name):
    return KSQ_LONG.get(name, (KSQ_NSQ, KSQ_MASK))


def kdec_record(name, a):
    """the record the decompression kernels see: z2 (and z3) zeroed for the exceptional branches"""
    r = list(a)
    if KDEC_BRANCH[name] >= 1:
        r[6] = r[7] = 0
    if KDEC_BRANCH[name] == 2:
        r[4] = r[5] = 0
    return r


def run_program(name, a, b=None):
    """one emulator run of a program on wire records a, b ([12] ints); -> wire result ([12] ints); the extremes go to cg.STATS"""
    kind, _, op = name.partition(":")
    if kind == "tower":
        return cg.Emu(wire_in=a, wire_in2=b).run(cg.prog_tower(op).steps).wire_out
    if kind == "tower2":
        return cg.Emu(wire_in=a, wire_in2=b).run(cg.prog_tower2(op).steps).wire_out
    if kind == "inv":
        prog_a = cg.prog_fexp_a(True) if op == "fp12" else cg.prog_tower_inv_a(op)
        ea = cg.Emu(wire_in=a).run(prog_a.steps)
        nn = cg.from_mont(ea.state[cg.ST_N])
        ea.state[cg.ST_NINV] = cg.mont(m.fp_inv(nn) if nn else 0)
        return cg.Emu(state=ea.state).run(cg.prog_tower_inv_b(op).steps).wire_out
    if kind == "kdec":
        a = kdec_record(name, a)
    st = cg.Emu(wire_in=a).run(cg.prog_tower_to_state(0 if kind == "ksq" else cg.ST_SNAP).steps).state
    if kind == "ksq":
        nsq, mask = ksq_params(name)
        cg.emu_ksq(st, 0, cg.ST_SNAP, nsq, mask)
        return [[cg.from_mont(st[cg.ST_SNAP + 12 * k + i]) if (cg.ST_SNAP + 12 * k + i) in st else None for i in range(12)]
                for k in range(bin(mask & ((1 << nsq) - 1)).count("1"))]
    cg.emu_kdec_a(st, cg.ST_SNAP, 1, cg.ST_KN)
    cg.emu_inv(st, cg.ST_KN, cg.ST_KNINV, 1)
    cg.emu_kdec_b(st, cg.ST_SNAP, 1, cg.ST_KNINV)
    return cg.Emu(state=st).run(cg.prog_tower_from_snap().steps).wire_out


def start_records(name, wa, wb):
    """the pool records a program starts from (and the CPU gate replays): (label, a, b)"""
    ra = adv.records(wa)
    if name in KSQ_LONG:
        ra = ra[::40]
    if not wb:
        return [(nm, a, None) for nm, a in ra]
    rb = adv.records(max(wb, 2))
    cut = lambda r: r[:wb] + [0] * (12 - wb)
    return [(nm, a, cut(rb[(5 * i + 1) % len(rb)][1])) for i, (nm, a) in enumerate(ra)]


def evaluate(name, a, b):
    cg.STATS = {}
    try:
        run_program(name, a, b)
        return dict(cg.STATS), None
    except AssertionError as ex:
        return dict(cg.STATS), str(ex) or "assertion"
    finally:
        cg.STATS = None


def mutate_fp(v, rng, pool_vals):
    k = rng.below(6)
    if k == 0:
        return pool_vals[rng.below(len(pool_vals))]
    if k == 1:
        return (v ^ (1 << rng.below(381))) % P
    if k == 2:
        return (P - 1 - v) % P
    # replace one 28-bit digit of the STORED (Montgomery, R = 2^392) representative by an extreme digit, map back to the wire
    s = v * adv.R28 % P
    i = rng.below(14)
    d = ((1 << 27) - 1, 1 << 27, 0, (1 << 28) - 1)[rng.below(4)]
    s = (s & ~(((1 << 28) - 1) << (28 * i)) | (d << (28 * i))) % P
    return s * pow(adv.R28, -1, P) % P


def mutate_record(a, b, wa, wb, rng, pool_vals):
    a, b = list(a), (None if b is None else list(b))
    if b is not None and rng.below(3) == 0:
        i = rng.below(wb)
        b[i] = a[rng.below(wa)] if rng.below(4) == 0 else mutate_fp(b[i], rng, pool_vals)
    else:
        i = rng.below(wa)
        a[i] = a[rng.below(wa)] if rng.below(4) == 0 else mutate_fp(a[i], rng, pool_vals)
    return a, b


def search_program(name, wa, wb, rng, pool_vals, findings):
    best = {}                                        # target -> (value, label, a, b)

    def note(label, a, b):
        st, err = evaluate(name, a, b)
        if err:
            findings.append({"program": name, "label": label, "error": err, "a": a, "b": b})
        for t in EMU_TARGETS:
            if st.get(t, 0) > best.get(t, (0,))[0]:
                best[t] = (st[t], label, a, b)
        return st

    for label, a, b in start_records(name, wa, wb):
        note(label, a, b)
    pool_max = {t: v[0] for t, v in best.items()}
    if name in KSQ_LONG:
        return best, pool_max
    serial = [0]

    def label():
        serial[0] += 1
        return "searched:%s:%d" % (name, serial[0])

    for t in EMU_TARGETS:
        if t not in best:
            continue                                 # the program never reaches that code
        for k in range(EVALS_PER_CLIMB):
            _, lab, a, b = best[t]
            na, nb = mutate_record(a, b, wa, wb, rng, pool_vals)
            note(label(), na, nb)
    # coordinate descent for the columns: every coefficient in turn takes each extreme stored digit pattern; the best stays
    ext = extremes()
    for t in ("max_col", "red_col"):
        for sweep in range(DESCENT_SWEEPS if t == "max_col" else 1):
            for side, w in (("a", wa), ("b", wb)):
                for i in range(w):
                    for x in ext:
                        _, lab, a, b = best[t]
                        na, nb = list(a), (None if b is None else list(b))
                        (na if side == "a" else nb)[i] = x
                        note(label(), na, nb)
    return best, pool_max


def sg_eval(g):
    tr = {}
    sgm.inv(g, packed=True, trace=tr)
    return {"batches": tr.get("batches", sgm.NB + 1), "de_hi": tr["de_hi"], "de_lo": -tr["de_lo"], "run_max": tr["run_max"], "entry_max": tr["entry_max"]}


def search_divsteps(rng, pool_ops):
    best = {}

    def note(label, g):
        st = sg_eval(g)
        for t in SG_TARGETS:
            if st[t] > best.get(t, [(0,)])[0][0]:
                best[t] = ([(st[t], label, g)] + best.get(t, []))[:3]
        return st

    for o in pool_ops:
        if o.v:
            note("%s:%s" % (o.cls, o.name), o.v)
    pool_max = {t: v[0][0] for t, v in best.items()}
    vals = [o.v for o in pool_ops]
    for t in SG_TARGETS:
        for k in range(EVALS_DIVSTEP):
            g = best[t][0][2]
            j = rng.below(4)
            if j == 0:
                ng = (g ^ (1 << rng.below(381))) % P
            elif j == 1:                             # one 30-bit limb replaced by an extreme
                i = rng.below(13)
                ng = (g & ~(sgm.M30 << (30 * i)) | ((0, sgm.M30, 1 << 29, 1)[rng.below(4)] << (30 * i))) % P
            elif j == 2:
                ng = (g + vals[rng.below(len(vals))]) % P
            else:
                ng = (g << (1 + rng.below(30))) % P
            if ng:
                note("searched:divsteps:%s:%d" % (t, k), ng)
    return best, pool_max


def hx(v):
    return "%x" % v


def main():
    t0 = time.time()
    rng = adv._Rng(SEED)
    pool_ops = adv.pool()
    pool_vals = [o.v for o in pool_ops]
    findings = []
    cg.COL_LIMIT_BITS = 63      # measure up to the hard limit: a canonical input between 2^62 and 2^63 is reported, not refused
    out = {"header": {"seed": SEED, "descent_sweeps": DESCENT_SWEEPS, "evals_per_climb": EVALS_PER_CLIMB, "evals_divstep": EVALS_DIVSTEP, "ksq": [KSQ_NSQ, KSQ_MASK],
                      "note": "maxima are what the pool and the search reached: lower bounds on the true worst case, not proofs",
                      "hard_limits": {"column": "< 2^63 (int64)", "limb": "< 2^31 (int32)", "q": "<= 14", "matrix_half": "int16",
                                      "mul24_operand": "24 signed bits", "batches": sgm.NB}},
           "maxima": {}, "pool_maxima": {}, "vectors": [], "divsteps": []}
    seen = {}
    for name, (wa, wb) in programs().items():
        best, pool_max = search_program(name, wa, wb, rng, pool_vals, findings)
        out["maxima"][name] = {t: v[0] for t, v in best.items()}
        out["pool_maxima"][name] = pool_max
        for t, (val, label, a, b) in best.items():
            if not label.startswith("searched:"):
                continue                             # a pool record holds the maximum: the gate replays the pool anyway
            key = (name, tuple(a), None if b is None else tuple(b))
            if key in seen:
                seen[key]["targets"][t] = val
                continue
            vec = {"program": name, "label": label, "targets": {t: val}, "a": [hx(x) for x in a]}
            if b is not None:
                vec["b"] = [hx(x) for x in b]
            seen[key] = vec
            out["vectors"].append(vec)
        print("%-18s %s" % (name, {t: (v.bit_length() if t in ("max_col", "red_col", "wn_limb") else round(v, 4) if isinstance(v, float) else v)
                                   for t, v in out["maxima"][name].items()}), flush=True)
    best, pool_max = search_divsteps(rng, pool_ops)
    out["maxima"]["divsteps"] = {t: v[0][0] for t, v in best.items()}
    out["pool_maxima"]["divsteps"] = pool_max
    for t, lst in best.items():
        for val, label, g in lst:
            out["divsteps"].append({"target": t, "value": val, "label": label, "g": hx(g)})
    print("divsteps           %s" % out["maxima"]["divsteps"])
    out["findings"] = [{**f, "a": [hx(x) for x in f["a"]], "b": None if f["b"] is None else [hx(x) for x in f["b"]]} for f in findings]
    for f in findings:
        print("FINDING", f["program"], f["label"], f["error"])
    with open(adv.JSON_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d vectors, %d division-step values, %d findings, %.0f s" % (adv.JSON_PATH, len(out["vectors"]), len(out["divsteps"]), len(findings), time.time() - t0))


if __name__ == "__main__":
    main()
