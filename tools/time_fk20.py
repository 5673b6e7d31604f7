"""Times the G1 NTT and the FK20 proofs on one GPU and writes JSON.
  g1ntt   zkp_g1_ntt_batch_dev, forward and inverse, at 2^12 points per vector (1 and 16 vectors).  Per stage: the same number of points
          as vectors of TWO points run only the stage that multiplies nothing and the conversion, so (t(2^12) - t(2)) / 11 is one
          twiddled stage.
  phases  the calls FK20 is made of, each on its own at the sizes of N = 4096, n = 1: the Fr transform of 2N, 2N scalar multiplications
          (zkp_g1_mul_batch_dev: the same chain, plus the conversion FK20 skips), the G1 transforms of 2N (inverse: the public call also
          scales, which FK20 does not) and of N.  Proxies: the real phases share one workspace and skip the conversions between them.
  fk20    zkp_kzg_fk20_batch_dev end to end at N = 4096, n = 1 and n = 16, against the path the library had before: zkp_kzg_open_batch_dev
          of the same polynomial at all N domain points - N openings of N terms each, n calls for n polynomials.  The proofs of both
          routes are compared byte for byte first.
Resident tensors, HIP events, warmed up; the median of --reps runs, the alternatives alternating.
Usage: python tools/time_fk20.py [--reps R] [--what g1ntt,phases,fk20] [--log2-n 12] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x5EED0000000000000000000000000000000000000000000000000000C0FFEE


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


def _points(eng, exps):
    """[e] g1 for Python integers e != 0"""
    import numpy as np
    from zkvm_pairings_amd import synthetic
    sc = np.stack([synthetic.int_to_scalar(e % synthetic.R_ORDER) for e in exps])
    return eng.g1_mul(synthetic.G1_GENERATOR, sc)[0]


def _g1ntt_rows(eng, log2_n, reps, warmup):
    import torch
    from zkvm_pairings_amd import synthetic
    rows = []
    for n_vec in (1, 16):
        total = n_vec << log2_n
        pts = _t(eng, eng.g1_mul(synthetic.G1_GENERATOR, synthetic.scalars(0x61A7, total))[0])
        out, out_inf = torch.empty_like(pts), torch.empty(total, dtype=torch.uint8, device=pts.device)
        fwd = lambda: eng.g1_ntt(pts, log2_n, out=out, out_inf=out_inf)
        inv = lambda: eng.g1_ntt(pts, log2_n, inverse=True, out=out, out_inf=out_inf)
        pairs = lambda: eng.g1_ntt(pts, 1, out=out, out_inf=out_inf)
        for _ in range(warmup):
            fwd(), inv(), pairs()
        torch.cuda.synchronize()
        back, _ = eng.g1_ntt(*eng.g1_ntt(pts, log2_n)[:1], log2_n, inverse=True)
        assert torch.equal(back, pts)
        t_fwd, t_inv, t_pairs = _events([fwd, inv, pairs], reps)
        row = {"log2_n": log2_n, "n_vec": n_vec, "g1_ntt_ms": round(t_fwd, 3), "g1_ntt_inverse_ms": round(t_inv, 3),
               "first_and_out_ms": round(t_pairs, 3), "ms_per_twiddled_stage": round((t_fwd - t_pairs) / max(log2_n - 1, 1), 3),
               "scaling_ms": round(t_inv - t_fwd, 3)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def _fixtures(eng, log2_n, n):
    """the monomial setup, the FK20 setup, the Lagrange setup (bit-reversed) and n polynomials in both forms, all resident"""
    import numpy as np
    from zkvm_pairings_amd import synthetic
    r = synthetic.R_ORDER
    big_n = 1 << log2_n
    mono = _points(eng, [pow(TAU, k, r) for k in range(big_n)])
    w = synthetic.fr_root_of_unity(log2_n)
    scale = (pow(TAU, big_n, r) - 1) * pow(big_n, -1, r) % r
    dom, acc = [], 1
    for _ in range(big_n):
        dom.append(acc)
        acc = acc * w % r
    slot = [dom[synthetic.bit_reverse(i, log2_n)] for i in range(big_n)]
    lagrange = _points(eng, [scale * d % r * pow(TAU - d, -1, r) % r for d in slot])
    setup, setup_inf = eng.kzg_fk20_setup(_t(eng, mono), log2_n)
    coeffs = synthetic.scalars(0xF420, n * big_n)
    return dict(mono=_t(eng, mono), lagrange=_t(eng, lagrange), setup=setup, setup_inf=setup_inf, coeffs=_t(eng, coeffs),
                slots=_t(eng, np.stack([synthetic.int_to_scalar(d) for d in slot])))


def _phase_row(eng, log2_n, reps, warmup):
    import torch
    from zkvm_pairings_amd import synthetic
    big_n = 1 << log2_n
    fx = _fixtures(eng, log2_n, 1)
    fr2 = _t(eng, synthetic.scalars(0xC0EF, 2 * big_n))
    out2, inf2 = torch.empty_like(fx["setup"]), torch.empty(2 * big_n, dtype=torch.uint8, device=fx["setup"].device)
    out1, inf1 = torch.empty_like(fx["mono"]), torch.empty(big_n, dtype=torch.uint8, device=fx["setup"].device)
    calls = [lambda: eng.fr_ntt(fr2, log2_n + 1, bitrev=True),
             lambda: eng.g1_mul(fx["setup"], fr2),
             lambda: eng.g1_ntt(fx["setup"], log2_n + 1, inverse=True, bitrev=True, inf=fx["setup_inf"], out=out2, out_inf=inf2),
             lambda: eng.g1_ntt(fx["mono"], log2_n, out=out1, out_inf=inf1),
             lambda: eng.kzg_fk20_setup(fx["mono"], log2_n)]
    for _ in range(warmup):
        for fn in calls:
            fn()
    torch.cuda.synchronize()
    t = _events(calls, reps)
    row = {"log2_n": log2_n, "fr_ntt_2n_ms": round(t[0], 3), "g1_mul_2n_ms": round(t[1], 3), "g1_intt_2n_scaled_ms": round(t[2], 3),
           "g1_ntt_n_ms": round(t[3], 3), "fk20_setup_ms": round(t[4], 3)}
    print(json.dumps(row), flush=True)
    return row


def _fk20_row(eng, log2_n, n, reps, warmup):
    import torch
    big_n = 1 << log2_n
    fx = _fixtures(eng, log2_n, n)
    evals = eng.fr_ntt(fx["coeffs"], log2_n, bitrev=True)
    rep_evals = [evals[j * big_n:(j + 1) * big_n].unsqueeze(0).expand(big_n, big_n, 4).contiguous() for j in range(n)]   # polynomial j, once per point
    new = lambda: eng.kzg_fk20(fx["setup"], fx["setup_inf"], fx["coeffs"], log2_n, bitrev=True)

    def old():
        return [eng.kzg_open(fx["lagrange"], ev, fx["slots"], log2_n, bitrev=True) for ev in rep_evals]

    for _ in range(warmup):
        new(), old()
    torch.cuda.synchronize()
    proof, inf = new()
    base = old()
    for j in range(n):
        assert torch.equal(base[j][0], evals[j * big_n:(j + 1) * big_n])
        assert torch.equal(base[j][1], proof[j * big_n:(j + 1) * big_n]) and torch.equal(base[j][2], inf[j * big_n:(j + 1) * big_n])
    t_new, t_old = _events([new, old], reps)
    row = {"log2_n": log2_n, "n": n, "fk20_ms": round(t_new, 3), "open_at_every_point_ms": round(t_old, 3), "old_over_new": round(t_old / t_new, 2),
           "us_per_proof": round(t_new * 1e3 / (n * big_n), 2)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--what", default="g1ntt,phases,fk20")
    ap.add_argument("--log2-n", type=int, default=12)
    ap.add_argument("--n", default="1,16")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    what = args.what.split(",")
    res = {"device": eng.device_info(), "g1ntt": [], "phases": [], "fk20": []}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    if "g1ntt" in what:
        res["g1ntt"] = _g1ntt_rows(eng, args.log2_n, args.reps, args.warmup)
        save()
    if "phases" in what:
        res["phases"].append(_phase_row(eng, args.log2_n, args.reps, args.warmup))
        save()
    if "fk20" in what:
        for n in [int(x) for x in args.n.split(",")]:
            res["fk20"].append(_fk20_row(eng, args.log2_n, n, args.reps, args.warmup))
            save()
    eng.close()


if __name__ == "__main__":
    main()
