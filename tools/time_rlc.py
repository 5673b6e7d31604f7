"""Times the batch check by random linear combination (zkp_pairing_check_batch_rlc_dev) on one GPU against zkp_pairing_check_batch_dev on
the same checks expanded to k + s1 + s2 pairs each, and writes JSON.  Shapes: 3 free pairs per check (BASELINE config 4) at 2^14 and 2^18
checks; Groth16 (1 free pair + 3 fixed-G2 columns) at 2^14 and 2^18; BLS with public keys in G1 (1 free pair + 1 fixed-G1 column) at
2^18.  Every batch is valid by construction (the flag must be 1).  Resident tensors, HIP events, warmed up; the median of --reps runs,
the RLC call and the plain check alternating.  Phases: the same work through the public calls, each timed alone - is_valid of every
point, the endomorphism scaling of the free G1 points (next to zkp_g1_mul_batch_dev with 256-bit scalars on the same points), the column
MSMs, and the one-product check of the scaled free pairs.
Usage: python tools/time_rlc.py [--reps R] [--max-log L] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _limbs(ints, words=4):
    import numpy as np
    return np.frombuffer(b"".join(int(v).to_bytes(8 * words, "little") for v in ints), dtype=np.uint64).reshape(-1, words)


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


def _batch(eng, n, k, s1, s2, seed):
    """valid checks: free pairs ([x_j]G1, [y_j]G2), fixed-G2 columns ([c_j]G1, [d_j]G2), fixed-G1 columns ([e_j]G1, [f_j]G2) with
    sum x y + sum c d + sum e f = 0 per check (the first free x, or the first column's c / f when k = 0, solved for)"""
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    rng = random.Random(seed)
    dev = torch.device("cuda", eng.device)
    d = [rng.randrange(1, R) for _ in range(s2)]
    e = [rng.randrange(1, R) for _ in range(s1)]
    xs, ys, cs, fs = [], [], [], []
    for _ in range(n):
        x = [rng.randrange(1, R) for _ in range(k)]
        y = [rng.randrange(1, R) for _ in range(k)]
        c = [rng.randrange(1, R) for _ in range(s2)]
        f = [rng.randrange(1, R) for _ in range(s1)]
        rest = sum(a * b for a, b in zip(x[1:], y[1:])) + sum(a * b for a, b in zip(c, d)) + sum(a * b for a, b in zip(e, f))
        x[0] = (-rest * pow(y[0], -1, R)) % R
        xs += x
        ys += y
        cs += c
        fs += f
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)
    g1 = lambda ks: eng.g1_mul(t(synthetic.G1_GENERATOR), t(_limbs(ks)))[0] if ks else None
    g2 = lambda ks: eng.g2_mul(t(synthetic.G2_GENERATOR), t(_limbs(ks)))[0] if ks else None
    return dict(g1=g1(xs), g2=g2(ys), k=k, col_g1=g1(cs), fixed_g2=g2(d), col_g2=g2(fs), fixed_g1=g1(e))


def _expand(b, n):
    import torch
    k = b["k"]
    parts1, parts2 = [], []
    if k:
        parts1.append(b["g1"].view(n, k, 12)), parts2.append(b["g2"].view(n, k, 24))
    if b["fixed_g2"] is not None:
        s2 = b["fixed_g2"].numel() // 24
        parts1.append(b["col_g1"].view(n, s2, 12)), parts2.append(b["fixed_g2"].view(1, s2, 24).expand(n, s2, 24))
    if b["fixed_g1"] is not None:
        s1 = b["fixed_g1"].numel() // 12
        parts1.append(b["fixed_g1"].view(1, s1, 12).expand(n, s1, 12)), parts2.append(b["col_g2"].view(n, s1, 24))
    e1, e2 = torch.cat(parts1, 1).contiguous(), torch.cat(parts2, 1).contiguous()
    return e1.view(-1, 12), e2.view(-1, 24), e1.shape[1]


def _row(eng, name, n, k, s1, s2, reps, warmup):
    import numpy as np
    import torch
    b = _batch(eng, n, k, s1, s2, seed=n + 31 * k + 7 * s1 + 3 * s2)
    e1, e2, kk = _expand(b, n)
    dev = torch.device("cuda", eng.device)
    rand = torch.from_numpy(eng.rlc_random(n).view(np.int64)).to(dev)
    rlc = lambda pc=False: eng.pairing_check_rlc(**b, rand=rand, points_checked=pc)
    plain = lambda: eng.pairing_check(e1, e2, kk)
    for _ in range(warmup):
        rlc(), rlc(True), plain()
    torch.cuda.synchronize()
    flag = int(rlc().item())
    _, allok = plain()
    assert flag == 1 and int(allok.item()) == 1, (name, n, flag)
    t_rlc, t_rlc_pc, t_plain = _events([rlc, lambda: rlc(True), plain], reps)
    # phases, each alone
    ph = {}
    pts = [(1, x) for x in (b["g1"], b["col_g1"], b["fixed_g1"]) if x is not None] + [(2, x) for x in (b["g2"], b["fixed_g2"], b["col_g2"]) if x is not None]
    ph["points_check"] = _events([lambda: [(eng.g1_is_valid if w == 1 else eng.g2_is_valid)(x) for w, x in pts]], reps)[0]
    if k:
        ab = rand.view(n, 2).repeat_interleave(k, 0).contiguous()
        sc = torch.zeros((n * k, 4), dtype=torch.int64, device=dev)
        sc[:, :2] = ab      # a 128-bit scalar per point: what the 256-bit kernel would be handed (it walks all 256 bits anyway)
        ph["scale_endo"], ph["scale_g1_mul_256"] = _events([lambda: eng.g1_mul_endo(b["g1"], ab), lambda: eng.g1_mul(b["g1"], sc)], reps)
        scaled, _ = eng.g1_mul_endo(b["g1"], ab)
        ph["free_pairs_product_check"] = _events([lambda: eng.pairing_product_check(scaled, b["g2"])], reps)[0]
    sc4 = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    sc4[:, :2] = rand.view(n, 2)
    if s2:
        col = b["col_g1"].view(n, s2, 12).transpose(0, 1).contiguous().view(-1, 12)
        ph["msm_g1_columns"] = _events([lambda: eng.g1_msm(col, sc4.repeat(s2, 1), s2)], reps)[0]
    if s1:
        col = b["col_g2"].view(n, s1, 24).transpose(0, 1).contiguous().view(-1, 24)
        ph["msm_g2_columns"] = _events([lambda: eng.g2_msm(col, sc4.repeat(s1, 1), s1)], reps)[0]
    row = {"shape": name, "n_checks": n, "k": k, "s1": s1, "s2": s2, "rlc_ms": round(t_rlc, 2), "rlc_points_checked_ms": round(t_rlc_pc, 2),
           "pairing_check_ms": round(t_plain, 2), "speedup": round(t_plain / t_rlc, 2), "speedup_points_checked": round(t_plain / t_rlc_pc, 2),
           "phases_ms": {a: round(v, 2) for a, v in ph.items()}}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-log", type=int, default=18)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    shapes = [("free3", 3, 0, 0, (14, 18)), ("groth16", 1, 0, 3, (14, 18)), ("bls_g1_keys", 1, 1, 0, (18,))]
    rows = []
    for name, k, s1, s2, logs in shapes:
        for lg in logs:
            if lg <= args.max_log:
                rows.append(_row(eng, name, 1 << lg, k, s1, s2, args.reps, args.warmup))
    res = {"device": eng.device_info(), "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
