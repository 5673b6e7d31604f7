"""Times the compressed-point path on one GPU with HIP events (warmed up; the variants alternate inside one process) and writes JSON:
  * decompression of 2^20 G1 and 2^20 G2 points (resident tensors), and compression of the same points
  * points_check_compressed against points_check on the same 2^20 pairs (k = 1), in alternating order
Usage: python tools/time_compressed.py [--n N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, reps):
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from zkvm_pairings_amd import PairingEngine, synthetic
    eng = PairingEngine(0)
    n = args.n
    g1, g2, _, _ = synthetic.random_pairs(eng, n, seed=0x7C0, device_tensors=True)
    c1, c2 = eng.compress_points_dev(g1, 1), eng.compress_points_dev(g2, 2)
    u1, u2 = eng.encode_points_dev(g1, 1), eng.encode_points_dev(g2, 2)
    dev = g1.device
    st1, st2 = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    ok, flag = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    variants = {
        "g1_decompress": lambda: eng.decompress_points_dev(c1, 1),
        "g2_decompress": lambda: eng.decompress_points_dev(c2, 2),
        "g1_compress": lambda: eng.compress_points_dev(g1, 1),
        "g2_compress": lambda: eng.compress_points_dev(g2, 2),
        "points_check": lambda: eng.points_check(u1, u2, 1, st1, st2, ok, flag),
        "points_check_compressed": lambda: eng.points_check_compressed(c1, c2, 1, st1, st2, ok, flag),
    }
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.reps):                        # alternate the variants: clock and thermal drift hit all of them alike
        for k, fn in variants.items():
            times[k] += _time(fn, 1)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    # the check's bytes agree (random pairs: every point valid, no check passes)
    eng.points_check_compressed(c1, c2, 1, st1, st2, ok, flag)
    torch.cuda.synchronize()
    agree = not st1.any().item() and not st2.any().item() and int(flag.item()) == 0
    res = {"n": n, "reps": args.reps, "device": eng.device_info(), "median_ms": med, "all_ms": times,
           "ms_per_2p20": {k: med[k] * (1 << 20) / n for k in med if "compress" in k and "check" not in k},
           "check_ratio_compressed_over_uncompressed": med["points_check_compressed"] / med["points_check"], "compressed_check_bytes_ok": agree}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
