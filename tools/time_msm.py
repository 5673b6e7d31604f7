"""Times the bucket MSM on one GPU and writes JSON: G1 and G2 MSMs of m terms (n_msm = 1, m = 2^10 .. 2^22, G2 up to --g2-max), and
2^14 sums of 64 terms over shared bases, each next to zkp_g*_mul_batch_dev on the same terms (the per-term multiplications alone, no
summation).  Resident tensors, HIP events, warmed up; the median of --reps runs.  The per-phase split (points, digits, sort, buckets,
reduce, final) comes from zkp_msm_profile_dev (one synchronised run per row).
Usage: python tools/time_msm.py [--reps R] [--max-log L] [--g2-max-log L] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ["points", "digits", "sort", "buckets", "reduce", "final"]


def _time(fn, reps):
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in evs)


def _row(eng, which, m, n_msm, shared, reps, warmup):
    import torch
    dev = torch.device("cuda", eng.device)
    from zkvm_pairings_amd import synthetic
    g = synthetic.G1_GENERATOR if which == 1 else synthetic.G2_GENERATOR
    import numpy as np
    n_pts = m if shared else m * n_msm
    # bases [a_i]G with 64-bit a_i, made on the device; scalars: uniform 256-bit integers
    a = torch.randint(1, 1 << 62, (n_pts, 4), dtype=torch.int64, device=dev)
    a[:, 1:] = 0
    mul = eng.g1_mul if which == 1 else eng.g2_mul
    pts, _ = mul(torch.from_numpy(np.asarray(g, dtype=np.uint64).view(np.int64)).to(dev), a)
    sc = torch.randint(-(1 << 63), (1 << 63) - 1, (m * n_msm, 4), dtype=torch.int64, device=dev)
    msm = eng.g1_msm if which == 1 else eng.g2_msm
    base = pts if not shared else pts.repeat(n_msm, 1)
    for _ in range(warmup):
        msm(pts, sc, n_msm, None, shared)
        mul(base, sc)
    torch.cuda.synchronize()
    t_msm = _time(lambda: msm(pts, sc, n_msm, None, shared), reps)
    t_mul = _time(lambda: mul(base, sc), reps)
    _, _, ph = eng.msm_profile(which, pts, sc, n_msm, shared)
    row = {"group": "G%d" % which, "m": m, "n_msm": n_msm, "shared": bool(shared), "terms": m * n_msm, "msm_ms": round(t_msm, 3),
           "mul_batch_ms": round(t_mul, 3), "speedup": round(t_mul / t_msm, 2), "phases_ms": {k: round(v, 3) for k, v in zip(PHASES, ph)}}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--min-log", type=int, default=10)
    ap.add_argument("--max-log", type=int, default=22)
    ap.add_argument("--g2-max-log", type=int, default=22)
    ap.add_argument("--step", type=int, default=2, help="log2 step between the sizes")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    rows = []
    for which in (1, 2):
        top = args.max_log if which == 1 else min(args.max_log, args.g2_max_log)
        for lg in range(args.min_log, top + 1, args.step):
            rows.append(_row(eng, which, 1 << lg, 1, False, args.reps, args.warmup))
        rows.append(_row(eng, which, 64, 1 << 14, True, args.reps, args.warmup))
    res = {"device": eng.device_info(), "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
