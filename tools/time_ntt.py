"""Times the batched Fr NTT and the KZG opening on one GPU and writes JSON.
  ntt   zkp_fr_ntt_batch_dev, forward, natural order and ZKP_NTT_BITREV, at 2^12 points (16, 256 and 4096 polynomials), 2^16 and 2^20
        (one polynomial), against the only route the library offered before: the same N/2 log2 N n_poly Montgomery products pushed
        through zkp_fr_op_batch_dev(ZKP_FR_MUL), log2 N calls of N/2 n_poly products each.  That route is given every advantage: its
        additions, its permutations and its twiddle gathers are left out.
  open  zkp_kzg_open_batch_dev on 4096-point polynomials (bit-reversed order), 16, 256 and 4096 per call, against the same work composed
        from the earlier calls: fr_eval on the device, the quotient on the host in Python integers (one batched inversion per
        polynomial), then the shared-bases g1_msm.  The host route is timed by the wall clock up to --host-max polynomials.
Resident tensors, HIP events, warmed up; the median of --reps runs, the alternatives alternating.
Usage: python tools/time_ntt.py [--reps R] [--what ntt,open] [--host-max 256] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def _scalars(seed, n):
    import numpy as np
    from zkvm_pairings_amd import synthetic
    base = synthetic.scalars(seed, min(n, 1 << 16))
    return np.ascontiguousarray(np.tile(base, (n // base.shape[0], 1)))


def _ntt_row(eng, log2_n, n_poly, reps, warmup):
    import torch
    total = n_poly << log2_n
    x = _t(eng, _scalars(0x177, total))
    y = torch.empty_like(x)
    half_a, half_b, half_o = x[:total // 2], x[total // 2:], torch.empty_like(x[:total // 2])
    nat = lambda: eng.fr_ntt(x, log2_n, out=y)
    brv = lambda: eng.fr_ntt(x, log2_n, bitrev=True, out=y)

    def old():
        for _ in range(log2_n):
            eng._chk(eng._lib.zkp_fr_op_batch_dev(eng._h, 0, eng._tp(half_a), eng._tp(half_b), total // 2, eng._tp(half_o), eng._stream()))

    for _ in range(warmup):
        nat(), brv(), old()
    torch.cuda.synchronize()
    back = eng.fr_ntt(eng.fr_ntt(x, log2_n), log2_n, inverse=True)
    assert torch.equal(back, x)
    t_nat, t_brv, t_old = _events([nat, brv, old], reps)
    products = (total // 2) * log2_n
    row = {"log2_n": log2_n, "n_poly": n_poly, "ntt_ms": round(t_nat, 4), "ntt_bitrev_ms": round(t_brv, 4), "fr_op_mul_route_ms": round(t_old, 4),
           "products_per_s": round(products / (t_nat * 1e-3)), "products_per_s_bitrev": round(products / (t_brv * 1e-3)),
           "old_over_new": round(t_old / t_nat, 2), "old_over_new_bitrev": round(t_old / t_brv, 2)}
    print(json.dumps(row), flush=True)
    return row


def _host_quotient(evals, z, y, log2_n):
    """q_i = (f_i - y) / (w^idx(i) - z) on Python integers, bit-reversed slots, one inversion per polynomial (Montgomery's trick); z is
    outside the domain here"""
    from zkvm_pairings_amd import synthetic
    r = synthetic.R_ORDER
    n = 1 << log2_n
    w = synthetic.fr_root_of_unity(log2_n)
    dom, acc = [], 1
    for _ in range(n):
        dom.append(acc)
        acc = acc * w % r
    slot = [dom[synthetic.bit_reverse(i, log2_n)] for i in range(n)]
    out = []
    for f, zz, yy in zip(evals, z, y):
        den = [(d - zz) % r for d in slot]
        pre, acc = [], 1
        for d in den:
            pre.append(acc)
            acc = acc * d % r
        inv = pow(acc, -1, r)
        q = [0] * n
        for i in range(n - 1, -1, -1):
            q[i] = (f[i] - yy) * (inv * pre[i] % r) % r
            inv = inv * den[i] % r
        out.append(q)
    return out


def _open_row(eng, n, reps, warmup, host_max):
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    log2_n = 12
    big_n = 1 << log2_n
    setup = _t(eng, eng.g1_mul(synthetic.G1_GENERATOR, synthetic.scalars(0x5E7, big_n))[0])      # any valid points time the same
    ev_host = _scalars(0xE7A, n * big_n)
    z_host = synthetic.scalars(0xE7B, n)
    ev, z = _t(eng, ev_host), _t(eng, z_host)
    new = lambda: eng.kzg_open(setup, ev, z, log2_n, bitrev=True)
    for _ in range(warmup):
        new()
    torch.cuda.synchronize()
    (t_new,) = _events([new], reps)
    row = {"n": n, "log2_n": log2_n, "kzg_open_ms": round(t_new, 3), "us_per_opening": round(t_new * 1e3 / n, 2)}
    if n <= host_max:
        ints = lambda a: [synthetic.scalar_to_int(v) for v in a]
        ts = []
        for _ in range(min(reps, 3)):
            t0 = time.perf_counter()
            y = eng.fr_eval(ev, z, log2_n, bitrev=True).cpu().numpy().view(np.uint64)
            f = ints(ev_host)
            q = _host_quotient([f[j * big_n:(j + 1) * big_n] for j in range(n)], ints(z_host), ints(y), log2_n)
            qs = _t(eng, np.stack([synthetic.int_to_scalar(v) for row_ in q for v in row_]))
            proofs, inf = eng.g1_msm(setup, qs, n, shared_bases=True)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        _, p_new, i_new = new()
        assert torch.equal(p_new, proofs) and torch.equal(i_new, inf)
        row["eval_host_quotient_msm_wall_ms"] = round(statistics.median(ts), 1)
        row["old_over_new"] = round(row["eval_host_quotient_msm_wall_ms"] / t_new, 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--what", default="ntt,open")
    ap.add_argument("--host-max", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    what = args.what.split(",")
    res = {"device": eng.device_info(), "ntt": [], "open": []}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    if "ntt" in what:
        for lg, n_poly in ((12, 16), (12, 256), (12, 4096), (16, 1), (20, 1)):
            res["ntt"].append(_ntt_row(eng, lg, n_poly, args.reps, args.warmup))
            save()
    if "open" in what:
        for n in (16, 256, 4096):
            res["open"].append(_open_row(eng, n, args.reps, args.warmup, args.host_max))
            save()
    eng.close()


if __name__ == "__main__":
    main()
