"""Times the cell recovery on one GPU and writes JSON.
  check     before any timing, at the timed shape: zkp_das_recover_batch_dev gives back the coefficients the cells were made from, ok = 1
            for every blob, and the composed baseline below gives the same bytes.
  recover   zkp_das_recover_batch_dev end to end at N = 2^log2_n, cells of 2^log2_l (PeerDAS: 4096, 64), a random half of the cells of
            every blob missing, for each n.
  composed  the same recovery out of calls the library had before: the textbook decoder on the D = 2 N points of the extended blob -
            E Z (zkp_fr_op_batch_dev), the inverse transform of size D, the forward transform on the coset, the product with 1 / Z, the
            inverse coset transform: three zkp_fr_ntt_batch_dev of size D and two products.  Its two Z tables (Z(X^l) on the D-th roots
            and its inverses on the coset) are computed OUTSIDE the timed region, which favours it; the new call builds Z, both tables
            and the inversion inside.
Resident tensors, HIP events, warmed up; the median of --reps runs, the two alternating rep by rep.
Usage: python tools/time_recover.py [--reps R] [--n 1,16,256] [--log2-n 12] [--log2-l 6] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _z_tables(eng, present, log2_n, log2_l):
    """Z_j(X^l) on the D-th roots (bit-reversed order, zero on the missing cells) and 1 / Z_j(X^l) on the coset, resident: the
    coefficients on Python integers, the evaluations by the library's transform"""
    import numpy as np
    from zkvm_pairings_amd import synthetic
    r = synthetic.R_ORDER
    n, big_m = present.shape
    mu, l, big_d = log2_n + 1 - log2_l, 1 << log2_l, 2 << log2_n
    w = synthetic.fr_root_of_unity(mu)
    roots = [pow(w, synthetic.bit_reverse(m, mu), r) for m in range(big_m)]
    zd = np.zeros((n, big_d, 4), dtype=np.uint64)
    for j in range(n):
        z = [1]
        for m in range(big_m):
            if not present[j, m]:
                z = [((z[d - 1] if d else 0) - roots[m] * (z[d] if d < len(z) else 0)) % r for d in range(len(z) + 1)]
        zd[j, 0:len(z) * l:l] = np.stack([synthetic.int_to_scalar(v) for v in z])
    zd = _t(eng, zd.reshape(-1, 4))
    on_roots = eng.fr_ntt(zd, log2_n + 1, bitrev=True)
    on_coset = eng.fr_ntt(zd, log2_n + 1, bitrev=True, coset=True)
    return on_roots, eng.fr_invert(on_coset, out=on_coset)


def measure(log2_n, log2_l, ns, reps, warmup):
    import numpy as np
    import torch
    from zkvm_pairings_amd import PairingEngine, synthetic
    eng = PairingEngine(0)
    big_n, big_d = 1 << log2_n, 2 << log2_n
    res = {"device": eng.device_info(), "log2_n": log2_n, "log2_l": log2_l, "rows": []}
    for n in ns:
        values, present, coeffs = synthetic.das_recover_instance(0xDA5 + n, n, log2_n, log2_l, bitrev=True, engine=eng)
        zeroed = values.copy()
        zeroed[present == 0] = 0                         # the composed route multiplies the missing cells by Z = 0: give it zeros to read
        d_values, d_present, d_zeroed = _t(eng, values.reshape(-1, 4)), _t(eng, present.reshape(-1)), _t(eng, zeroed.reshape(-1, 4))
        z_roots, z_coset_inv = _z_tables(eng, present, log2_n, log2_l)
        lg = log2_n + 1

        def recover():
            return eng.das_recover(d_values, d_present, log2_n, log2_l, True)

        def composed():
            x = eng.fr_op("mul", d_zeroed, z_roots)
            eng.fr_ntt(x, lg, inverse=True, bitrev=True, out=x)
            eng.fr_ntt(x, lg, bitrev=True, coset=True, out=x)
            x = eng.fr_op("mul", x, z_coset_inv)
            return eng.fr_ntt(x, lg, inverse=True, bitrev=True, coset=True, out=x)

        for _ in range(warmup):
            recover(), composed()
        torch.cuda.synchronize()
        got, ok = recover()
        want = coeffs.reshape(-1, 4).tobytes()
        assert got.cpu().numpy().view(np.uint64).tobytes() == want and bool((ok == 1).all()), "the recovery does not give the polynomials back"
        base = composed().cpu().numpy().view(np.uint64).reshape(n, big_d, 4)
        assert base[:, :big_n].tobytes() == want and not base[:, big_n:].any(), "the composed baseline does not give the polynomials back"
        inner = max(1, 64 // n)                          # calls per timed window: a window of one small call would measure the launch queue
        t = [v / inner for v in _events([lambda: [recover() for _ in range(inner)], lambda: [composed() for _ in range(inner)]], reps)]
        row = {"n": n, "calls_per_window": inner, "recover_ms": round(t[0], 4), "composed_ms": round(t[1], 4), "composed_over_recover": round(t[1] / t[0], 2),
               "us_per_blob": round(t[0] * 1e3 / n, 2), "input_gb_per_s": round(n * big_d * 32 / (t[0] * 1e6), 1)}
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2-n", type=int, default=12)
    ap.add_argument("--log2-l", type=int, default=6)
    ap.add_argument("--n", default="1,16,256")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    res = measure(args.log2_n, args.log2_l, [int(x) for x in args.n.split(",")], args.reps, args.warmup)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
