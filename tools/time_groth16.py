"""Times the batched Groth16 verifier (zkp_groth16_verify_batch_dev) on one GPU and writes JSON.  For n in {2^10, 2^14, 2^18} proofs and
n_inputs in {1, 8, 64}:
  (a) the call itself, with default flags and with both CHECKED flags;
  (b) the route through the calls that do not know Groth16: every vk_x_c by zkp_g1_msm_batch_dev with shared bases (the scalar 1 for
      IC_0), then zkp_pairing_check_batch_rlc_dev with one free pair and three fixed-G2 columns (alpha, vk_x_c, C_c against -beta, -gamma,
      -delta);
  (c) groth16_verify_each, the per-proof path (host arrays, wall clock);
  (d) zkp_fr_fold_batch_dev alone.
Every batch is valid by construction (synthetic.groth16_instance on at most 1024 proofs, tiled to n: the flag must be 1).  Resident
tensors, HIP events, warmed up; the median of --reps runs, (a), (b) and (d) alternating.
Usage: python tools/time_groth16.py [--reps R] [--logs 10,14,18] [--inputs 1,8,64] [--no-each] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = 1024


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


def _row(eng, n, l, reps, warmup, each):
    import numpy as np
    import torch
    from zkvm_pairings_amd import Groth16VerifyingKey, groth16_verify_each, synthetic
    from zkvm_pairings_amd.pairings import _g2_neg_array
    dev = torch.device("cuda", eng.device)
    nb = min(n, BASE)
    key, (a, b, c), x = synthetic.groth16_instance(0x7160 + 64 * l + nb, nb, l, engine=eng)
    vk = Groth16VerifyingKey(*key)
    tile = lambda arr: np.ascontiguousarray(np.tile(arr, (n // nb,) + (1,) * (arr.ndim - 1)))
    a, b, c, x = tile(a), tile(b), tile(c), tile(x)
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to(dev)
    tk = [t(v) for v in vk.arrays()]
    ta, tb, tc, tx = t(a), t(b), t(c), t(x.reshape(-1, 4))
    rand = t(eng.rlc_random(n))
    new = lambda checked=False: eng.groth16_verify_batch(*tk, ta, tb, tc, tx, rand=rand, points_checked=checked, vk_checked=checked)
    # (b): the scalars of the n shared-base sums, the fixed G2 points negated once (they belong to the key)
    sc = torch.zeros((n, l + 1, 4), dtype=torch.int64, device=dev)
    sc[:, 0, 0] = 1
    sc[:, 1:] = tx.view(n, l, 4)
    fixed = t(np.stack([_g2_neg_array(vk.beta_g2), _g2_neg_array(vk.gamma_g2), _g2_neg_array(vk.delta_g2)]))
    alpha = tk[0].view(1, 12).expand(n, 12)
    step = max(1, (1 << 24) // (l + 1))                    # the MSM's limit on m * n_msm

    def old():
        parts = [eng.g1_msm(tk[4], sc[lo:lo + step].reshape(-1, 4), min(step, n - lo), shared_bases=True)[0] for lo in range(0, n, step)]
        vkx = parts[0] if len(parts) == 1 else torch.cat(parts)
        col = torch.stack([alpha, vkx, tc], 1).contiguous().view(-1, 12)
        return eng.pairing_check_rlc(ta, tb, 1, col_g1=col, fixed_g2=fixed, rand=rand)

    sw = sc[:, 0].contiguous()                             # any canonical weights do for (d): the 1s are replaced by the scalars' shape
    sw[:, :2] = rand.view(n, 2)
    fold = lambda: eng.fr_fold(sw, tx, l)
    for _ in range(warmup):
        new(), new(True), old(), fold()
    torch.cuda.synchronize()
    assert int(new().item()) == 1 and int(new(True).item()) == 1 and int(old().item()) == 1, (n, l)
    t_new, t_chk, t_old, t_fold = _events([new, lambda: new(True), old, fold], reps)
    row = {"n": n, "n_inputs": l, "verify_batch_ms": round(t_new, 2), "verify_batch_checked_ms": round(t_chk, 2), "msm_plus_rlc_ms": round(t_old, 2),
           "fr_fold_ms": round(t_fold, 3), "old_over_new": round(t_old / t_new, 2)}
    if each:
        groth16_verify_each(vk, (a, b, c), x, engine=eng)
        ts = []
        for _ in range(min(reps, 3)):
            t0 = time.perf_counter()
            ok = groth16_verify_each(vk, (a, b, c), x, engine=eng)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert ok.all()
        row["verify_each_wall_ms"] = round(statistics.median(ts), 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--logs", default="10,14,18")
    ap.add_argument("--inputs", default="1,8,64")
    ap.add_argument("--no-each", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    rows = []
    for lg in [int(v) for v in args.logs.split(",")]:
        for l in [int(v) for v in args.inputs.split(",")]:
            rows.append(_row(eng, 1 << lg, l, args.reps, args.warmup, not args.no_each))
            if args.out:
                with open(args.out, "w") as f:
                    json.dump({"device": eng.device_info(), "rows": rows}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
