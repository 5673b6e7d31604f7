"""Times the batched Fr inversion, the barycentric evaluation and the batch KZG opening verifier on one GPU and writes JSON.
  invert  zkp_fr_invert_batch_dev against zkp_fr_op_batch_dev(ZKP_FR_INVERT) at n = 2^12, 2^16, 2^20, 2^24;
  eval    zkp_fr_eval_batch_dev for 2^4, 2^8, 2^12 polynomials of 4096 evaluations (bit-reversed order);
  kzg     for n in {2^10, 2^14, 2^18} openings:
    (a) zkp_kzg_verify_batch_dev with default flags and with both CHECKED flags;
    (b) the route through the calls that do not know KZG: C_i - [y_i] g1 + [z_i] pi_i by two scalar multiplications and two additions
        per opening, then zkp_pairing_check_batch_rlc_dev with no free pair and two fixed-G2 columns (-g2, [tau] g2);
    (c) kzg_verify_each, the per-opening path (host arrays, wall clock);
    (s) the verifier's two sums formed both ways through the public MSM call: ONE shared-bases call over C | pi | g1 with rows
        r | t | -u and 0 | r | 0 (what the verifier does), against two calls of 2 n + 1 and n terms.
Every batch is valid by construction (synthetic.kzg_instance on at most 1024 openings, tiled to n: the flag must be 1).  Resident
tensors, HIP events, warmed up; the median of --reps runs, the alternatives alternating.
Usage: python tools/time_kzg.py [--reps R] [--what invert,eval,kzg] [--logs 10,14,18] [--no-each] [--out FILE]"""
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


def _t(eng, arr):
    import numpy as np
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to(torch.device("cuda", eng.device))


def _invert_row(eng, n, reps, warmup):
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    base = synthetic.scalars(0x1A7, min(n, 1 << 16))
    a = _t(eng, np.tile(base, (n // base.shape[0], 1)))
    new, old = lambda: eng.fr_invert(a), lambda: eng.fr_op("invert", a)
    for _ in range(warmup):
        new(), old()
    torch.cuda.synchronize()
    assert torch.equal(new(), old())
    t_new, t_old = _events([new, old], reps)
    row = {"n": n, "fr_invert_ms": round(t_new, 4), "fr_op_invert_ms": round(t_old, 4), "old_over_new": round(t_old / t_new, 2)}
    print(json.dumps(row), flush=True)
    return row


def _eval_row(eng, n_poly, reps, warmup):
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    base = synthetic.scalars(0xE7A, 16 * 4096)
    ev = _t(eng, np.tile(base, (n_poly // 16, 1)))
    z = _t(eng, synthetic.scalars(0xE7B, n_poly))
    fn = lambda: eng.fr_eval(ev, z, 12, bitrev=True)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    (t,) = _events([fn], reps)
    row = {"n_poly": n_poly, "log2_n": 12, "fr_eval_ms": round(t, 4), "ns_per_evaluation": round(t * 1e6 / (n_poly * 4096), 3)}
    print(json.dumps(row), flush=True)
    return row


def _kzg_row(eng, n, reps, warmup, each):
    import numpy as np
    import torch
    from zkvm_pairings_amd import KzgSetup, kzg_verify_each, synthetic
    from zkvm_pairings_amd.pairings import _g2_neg_array
    nb = min(n, BASE)
    key, c, z, y, p = synthetic.kzg_instance(0x7A60 + nb, nb, engine=eng)
    setup = KzgSetup(*key)
    tile = lambda arr: np.ascontiguousarray(np.tile(arr, (n // nb,) + (1,) * (arr.ndim - 1)))
    c, z, y, p = tile(c), tile(z), tile(y), tile(p)
    tk = [_t(eng, v) for v in setup.arrays()]
    tc, tz, ty, tp = _t(eng, c), _t(eng, z), _t(eng, y), _t(eng, p)
    rand = _t(eng, eng.rlc_random(n))
    new = lambda checked=False: eng.kzg_verify_batch(*tk, tc, tz, ty, tp, rand=rand, points_checked=checked, vk_checked=checked)
    fixed = _t(eng, np.stack([_g2_neg_array(setup.g2), setup.tau_g2]))

    def old():
        yg, yi = eng.g1_mul(tk[0], eng.fr_op("neg", ty))
        zp, zi = eng.g1_mul(tp, tz)
        s, si = eng.g1_add(tc, yg, None, yi)
        lhs, li = eng.g1_add(s, zp, si, zi)
        col = torch.stack([lhs, tp], 1).contiguous().view(-1, 12)
        ci = torch.stack([li, torch.zeros_like(li)], 1).contiguous().view(-1)
        return eng.pairing_check_rlc(None, None, 0, col_g1=col, col_inf1=ci, fixed_g2=fixed, rand=rand)

    # (s): the operands of the two sums as the verifier forms them - any canonical scalars time the same
    pts = torch.cat([tc, tp, tk[0].view(1, 12)])
    r = torch.zeros((n, 4), dtype=torch.int64, device=tc.device)
    r[:, :2] = rand.view(n, 2)
    zero1 = torch.zeros((1, 4), dtype=torch.int64, device=tc.device)
    row0 = torch.cat([r, tz, ty[:1]])
    shared_sc = torch.cat([row0, torch.zeros_like(r), r, zero1]).contiguous()
    shared = lambda: eng.g1_msm(pts, shared_sc, 2, shared_bases=True)
    two = lambda: (eng.g1_msm(pts, row0, 1), eng.g1_msm(tp, r, 1))
    for _ in range(warmup):
        new(), new(True), old(), shared(), two()
    torch.cuda.synchronize()
    assert int(new().item()) == 1 and int(new(True).item()) == 1 and int(old().item()) == 1, n
    (s_out, _), ((t0, _), (t1, _)) = shared(), two()
    assert torch.equal(s_out[0], t0[0]) and torch.equal(s_out[1], t1[0])
    t_new, t_chk, t_old, t_shared, t_two = _events([new, lambda: new(True), old, shared, two], reps)
    row = {"n": n, "verify_batch_ms": round(t_new, 3), "verify_batch_checked_ms": round(t_chk, 3), "points_plus_rlc_ms": round(t_old, 3),
           "old_over_new": round(t_old / t_new, 2), "sums_shared_bases_ms": round(t_shared, 3), "sums_two_calls_ms": round(t_two, 3)}
    if each:
        kzg_verify_each(setup, c, z, y, p, engine=eng)
        ts = []
        for _ in range(min(reps, 3)):
            t0 = time.perf_counter()
            ok = kzg_verify_each(setup, c, z, y, p, engine=eng)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert ok.all()
        row["verify_each_wall_ms"] = round(statistics.median(ts), 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--what", default="invert,eval,kzg")
    ap.add_argument("--logs", default="10,14,18")
    ap.add_argument("--no-each", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    what = args.what.split(",")
    res = {"device": eng.device_info(), "invert": [], "eval": [], "kzg": []}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    if "invert" in what:
        for lg in (12, 16, 20, 24):
            res["invert"].append(_invert_row(eng, 1 << lg, args.reps, args.warmup))
            save()
    if "eval" in what:
        for lg in (4, 8, 12):
            res["eval"].append(_eval_row(eng, 1 << lg, args.reps, args.warmup))
            save()
    if "kzg" in what:
        for lg in [int(v) for v in args.logs.split(",")]:
            res["kzg"].append(_kzg_row(eng, 1 << lg, args.reps, args.warmup, not args.no_each))
            save()
    eng.close()


if __name__ == "__main__":
    main()
