"""Times the KZG cell proofs on one GPU and writes JSON.
  check   before any timing: at l = 1 the proofs equal zkp_kzg_fk20_batch_dev's byte for byte; at the timed shape the batch verifier accepts
          every cell of the first polynomials, cells taken from the Fr transform of the zero-padded coefficients.
  cells   zkp_kzg_cells_batch_dev end to end at N = 2^log2_n, cells of 2^log2_l, extension 2 (PeerDAS: 4096, 64), for each n, against the
          parent's zkp_kzg_fk20_batch_dev on the same coefficients: the same 2 N base multiplications per polynomial without shared
          doublings, and transforms of 2 N and N instead of 2 k and M.
  groups  the producer's own time per group size g.  The library has no knob for g (the planner chooses it per call, zkp_cells_plan.hpp),
          so the override is local to this tool: `--prepare` (no GPU needed) copies the sources to build/time_cells/g<G>/, replaces the body
          of group_log2 in THAT copy by a constant and builds a private library there; the measurement then runs one child process per
          variant on its private copy of the package, and compares the SHA-256 of the proofs with the stock library's before it times.
Resident tensors, HIP events, warmed up; the median of --reps runs, the alternatives alternating.
Usage: python tools/time_cells.py --prepare            (once, after every change of the sources)
       python tools/time_cells.py [--reps R] [--n 1,16,256] [--log2-n 12] [--log2-l 6] [--out FILE]"""
import argparse
import hashlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = os.path.join(ROOT, "build", "time_cells")
TAU = 0x5EED0000000000000000000000000000000000000000000000000000C0FFEE
GROUPS = (1, 2, 4)


def prepare(jobs):
    """build/time_cells/g<G>/{include, zkvm_pairings_amd/*.py, zkvm_pairings_amd/csrc}: group_log2 returns min(log2 G, log2_l)"""
    procs = []
    for g in GROUPS:
        top = os.path.join(VARIANTS, "g%d" % g)
        shutil.rmtree(top, ignore_errors=True)
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(top, "include"))
        shutil.copytree(os.path.join(ROOT, "zkvm_pairings_amd"), os.path.join(top, "zkvm_pairings_amd"),
                        ignore=shutil.ignore_patterns("*.so", "__pycache__", "*.o"))
        plan = os.path.join(top, "zkvm_pairings_amd", "csrc", "zkp_cells_plan.hpp")
        with open(plan) as f:
            text = f.read()
        new, hits = re.subn(r"(ZKP_FK20_HD uint32_t group_log2\(size_t n_poly, unsigned log2_n, unsigned log2_l\) \{\n).*?\n\}\n",
                            lambda m: m.group(1) + "    (void)n_poly, (void)log2_n;\n    return %du < log2_l ? %du : log2_l;\n}\n" % (g.bit_length() - 1, g.bit_length() - 1),
                            text, count=1, flags=re.S)
        assert hits == 1, "group_log2 not found in zkp_cells_plan.hpp"
        with open(plan, "w") as f:
            f.write(new)
        procs.append((g, subprocess.Popen(["make", "-C", os.path.join(top, "zkvm_pairings_amd", "csrc")], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)))
        if len(procs) >= jobs:
            for g0, p in procs:
                assert p.wait() == 0, (g0, p.stderr.read()[-2000:])
            procs = []
    for g0, p in procs:
        assert p.wait() == 0, (g0, p.stderr.read()[-2000:])
    for g in GROUPS:                     # the measurement needs the library and the Python files, not the sources
        shutil.rmtree(os.path.join(VARIANTS, "g%d" % g, "zkvm_pairings_amd", "csrc"), ignore_errors=True)
        shutil.rmtree(os.path.join(VARIANTS, "g%d" % g, "include"), ignore_errors=True)
    print("variants built under %s: %s" % (VARIANTS, ", ".join("g%d" % g for g in GROUPS)))


def _events(calls, reps):
    """median ms of each call, the calls alternating rep by rep"""
    import torch
    evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in calls]
    for r in range(reps):
        for fn, ev in zip(calls, evs):
            ev[r][0].record()
            fn()
            ev[r][1].record()
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) for a, b in ev) for ev in evs]


def _t(eng, arr):
    import numpy as np
    import torch
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", eng.device))


def _powers(n):
    from zkvm_pairings_amd import synthetic
    out, acc = [], 1
    for _ in range(n):
        out.append(acc)
        acc = acc * TAU % synthetic.R_ORDER
    return out


def _points(eng, exps):
    import numpy as np
    from zkvm_pairings_amd import synthetic
    return eng.g1_mul(synthetic.G1_GENERATOR, np.stack([synthetic.int_to_scalar(e % synthetic.R_ORDER) for e in exps]))[0]


def _coeffs(n, log2_n):
    from zkvm_pairings_amd import synthetic
    return synthetic.scalars(0xCE11, n << log2_n)


def _digest(proof, inf):
    return hashlib.sha256(proof.cpu().numpy().tobytes() + inf.cpu().numpy().tobytes()).hexdigest()


def check(eng, mono, log2_n, log2_l, n):
    """bytes against FK20 at l = 1; the verifier's verdict on every cell of min(n, 2) polynomials at the timed shape"""
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    r, big_n, l = synthetic.R_ORDER, 1 << log2_n, 1 << log2_l
    coeffs = _t(eng, _coeffs(min(n, 2), log2_n))
    s1, i1 = eng.kzg_cells_setup(mono, log2_n, 0)
    f1, fi1 = eng.kzg_fk20_setup(mono, log2_n)
    assert torch.equal(s1, f1) and torch.equal(i1, fi1)
    a, ai = eng.kzg_cells(s1, i1, coeffs, log2_n, 0, 0, True)
    b, bi = eng.kzg_fk20(f1, fi1, coeffs, log2_n, True)
    assert torch.equal(a, b) and torch.equal(ai, bi), "cells of one value differ from the FK20 single proofs"
    st, sti = eng.kzg_cells_setup(mono, log2_n, log2_l)
    proof, inf = eng.kzg_cells(st, sti, coeffs, log2_n, log2_l, 1, True)
    n_poly, big_m = coeffs.shape[0] >> log2_n, (2 * big_n) // l
    padded = torch.zeros((n_poly, 2 * big_n, 4), dtype=coeffs.dtype, device=coeffs.device)
    padded[:, :big_n] = coeffs.reshape(n_poly, big_n, 4)
    values = eng.fr_ntt(padded.reshape(-1, 4), log2_n + 1, bitrev=True)
    pw = _powers(big_n)
    host = coeffs.cpu().numpy().view(np.uint64).reshape(n_poly, big_n, 4)
    com = _points(eng, [sum(c * p for c, p in zip(synthetic._ints(host[j]), pw)) % r for j in range(n_poly)])
    tg2 = eng.g2_mul(synthetic.G2_GENERATOR, np.stack([synthetic.int_to_scalar(pow(TAU, l, r))]))[0][0]
    idx = torch.arange(big_m, dtype=torch.int32, device=coeffs.device).repeat(n_poly)
    ok = eng.kzg_cell_verify(mono[:l].contiguous(), _t(eng, synthetic.G2_GENERATOR), _t(eng, tg2), _t(eng, np.repeat(com, big_m, axis=0)), idx, values, proof,
                             log2_n + 1, log2_l, bitrev=True, inf_proof=inf)
    assert int(ok.item()) == 1, "the batch verifier refuses what the producer made"
    values[5, 0] ^= 1
    bad = eng.kzg_cell_verify(mono[:l].contiguous(), _t(eng, synthetic.G2_GENERATOR), _t(eng, tg2), _t(eng, np.repeat(com, big_m, axis=0)), idx, values, proof,
                              log2_n + 1, log2_l, bitrev=True, inf_proof=inf)
    assert int(bad.item()) == 0
    return {"fk20_bytes_equal_at_l1": True, "cells_verified": n_poly * big_m}


def measure(log2_n, log2_l, ns, reps, warmup, with_fk20):
    """rows of one library (this process's): the producer, and FK20 on the same coefficients"""
    import torch
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    mono = _t(eng, _points(eng, _powers(1 << log2_n)))
    rows = {"device": eng.device_info(), "rows": []}
    if with_fk20:
        rows["check"] = check(eng, mono, log2_n, log2_l, max(ns))
        print(json.dumps(rows["check"]), flush=True)
        fs, fi = eng.kzg_fk20_setup(mono, log2_n)
    st, sti = eng.kzg_cells_setup(mono, log2_n, log2_l)
    for n in ns:
        coeffs = _t(eng, _coeffs(n, log2_n))
        calls = [lambda: eng.kzg_cells(st, sti, coeffs, log2_n, log2_l, 1, True)]
        if with_fk20:
            calls.append(lambda: eng.kzg_fk20(fs, fi, coeffs, log2_n, True))
        for _ in range(warmup):
            for fn in calls:
                fn()
        torch.cuda.synchronize()
        row = {"log2_n": log2_n, "log2_l": log2_l, "n": n, "sha256": _digest(*calls[0]())}
        t = _events(calls, reps)
        row["cells_ms"] = round(t[0], 3)
        row["us_per_proof"] = round(t[0] * 1e3 / (n * ((2 << log2_n) >> log2_l)), 2)
        if with_fk20:
            row["fk20_ms"] = round(t[1], 3)
            row["fk20_over_cells"] = round(t[1] / t[0], 2)
        print(json.dumps(row), flush=True)
        rows["rows"].append(row)
    eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--jobs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2-n", type=int, default=12)
    ap.add_argument("--log2-l", type=int, default=6)
    ap.add_argument("--n", default="1,16,256")
    ap.add_argument("--out", default="")
    ap.add_argument("--variant", default="", help="internal: the child process of one group size")
    args = ap.parse_args()
    if args.prepare:
        return prepare(args.jobs)
    ns = [int(x) for x in args.n.split(",")]
    if args.variant:                     # a child: the private copy of the package, no FK20 column
        sys.path.insert(0, os.path.join(VARIANTS, args.variant))
        import zkvm_pairings_amd
        assert os.path.dirname(os.path.abspath(zkvm_pairings_amd.__file__)).startswith(VARIANTS)
        print("RESULT " + json.dumps(measure(args.log2_n, args.log2_l, ns, args.reps, args.warmup, False)))
        return
    sys.path.insert(0, ROOT)
    res = {"stock": measure(args.log2_n, args.log2_l, ns, args.reps, args.warmup, True), "groups": {}}
    stock = {r["n"]: r for r in res["stock"]["rows"]}
    for g in GROUPS:
        name = "g%d" % g
        if g > 1 << args.log2_l or not os.path.exists(os.path.join(VARIANTS, name, "zkvm_pairings_amd", "libzkp_pairings.so")):
            continue                     # not admissible for the shape, or not prepared
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", name, "--reps", str(args.reps), "--warmup", str(args.warmup),
                              "--log2-n", str(args.log2_n), "--log2-l", str(args.log2_l), "--n", args.n], capture_output=True, text=True, timeout=900)
        if out.returncode:
            print(out.stdout[-2000:] + out.stderr[-2000:])
            raise SystemExit("variant %s failed: nothing further is started" % name)
        rows = json.loads([ln for ln in out.stdout.split("\n") if ln.startswith("RESULT ")][0][7:])["rows"]
        for r in rows:
            assert r["sha256"] == stock[r["n"]]["sha256"], "g = %d gives other proofs at n = %d" % (g, r["n"])
        res["groups"][name] = {r["n"]: r["cells_ms"] for r in rows}
        print(json.dumps({name: res["groups"][name]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
