"""Times hash-to-G2 and the BLS batch verifier on one GPU and writes JSON.
  check     before any timing: zkp_bls_verify_batch_dev accepts the instance and refuses it with one message changed.
  hash      zkp_hash_to_g2_batch_dev on n messages of 32 bytes, beside zkp_g2_decompress_batch_dev + zkp_g2_is_valid_batch_dev on n points:
            comparable field work (one Fp2 root and one 64-bit ladder per point), the yardstick of the map kernels; and
            zkp_hash_to_field_g2_batch_dev alone, the share of SHA-256 and the reductions.
  verify    zkp_bls_verify_batch_dev beside zkp_pairing_check_batch_rlc_dev on the same checks with the points already hashed (the
            difference is the hash), and beside zkp_pairing_check_batch_dev with k = 2.
Resident tensors, HIP events, warmed up; the median and the spread (min, max) of --reps runs, the calls alternating rep by rep.
Usage: python tools/time_bls.py [--reps R] [--hash-n 1024,65536,1048576] [--verify-n 1024,16384,262144] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"


def _events(calls, reps):
    """(median, min, max) ms of each call, the calls alternating rep by rep"""
    import torch
    evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in calls]
    for r in range(reps):
        for fn, ev in zip(calls, evs):
            ev[r][0].record()
            fn()
            ev[r][1].record()
    torch.cuda.synchronize()
    out = []
    for ev in evs:
        t = [a.elapsed_time(b) for a, b in ev]
        out.append(dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)))
    return out


def _t(eng, arr):
    import numpy as np
    import torch
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", eng.device))


def _messages(n, seed):
    import numpy as np
    from zkvm_pairings_amd import synthetic
    buf = synthetic.splitmix64(seed, 4 * n).view(np.uint8)
    return buf, np.arange(n + 1, dtype=np.uint64) * 32


def time_hash(eng, n, reps):
    import torch
    buf, off = _messages(n, 0x7A5)
    tb, to = _t(eng, buf), _t(eng, off)
    dst = torch.frombuffer(bytearray(DST), dtype=torch.uint8).to(tb.device)
    pts, inf = eng.hash_to_g2(tb, dst, offsets=to)                       # also grows the workspace
    comp = eng.compress_points_dev(pts, 2, inf)

    def yard():
        p, i, _ = eng.decompress_points_dev(comp, 2)
        eng.g2_is_valid(p, i)
    calls = [lambda: eng.hash_to_g2(tb, dst, offsets=to), yard, lambda: eng.hash_to_field_g2(tb, dst, offsets=to)]
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    res = _events(calls, reps)
    return dict(n=n, hash_to_g2=res[0], decompress_plus_is_valid=res[1], hash_to_field=res[2])


def time_verify(eng, n, reps):
    import torch
    from zkvm_pairings_amd import synthetic
    _, pks, msgs, sigs = synthetic.bls_instance(n, seed=0xB0B, engine=eng)
    buf, off = eng.pack_messages(msgs)
    tpk, tsig, tb, to = _t(eng, pks), _t(eng, sigs), _t(eng, buf), _t(eng, off)
    dst = torch.frombuffer(bytearray(DST), dtype=torch.uint8).to(tpk.device)
    rand = _t(eng, eng.rlc_random(n))
    assert int(eng.bls_verify(tpk, tb, tsig, dst, offsets=to, rand=rand).cpu()[0]) == 1, "the instance does not verify"
    bad = buf.copy()
    bad[0] ^= 1
    assert int(eng.bls_verify(tpk, _t(eng, bad), tsig, dst, offsets=to, rand=rand).cpu()[0]) == 0, "a changed message verifies"
    hq, hinf = eng.hash_to_g2(tb, dst, offsets=to)
    from zkvm_pairings_amd import G1Affine
    neg = _t(eng, (-G1Affine.generator()).to_array())
    g1 = torch.stack([tpk, neg.expand(n, 12)], dim=1).reshape(-1, 12).contiguous()
    g2 = torch.stack([hq, tsig], dim=1).reshape(-1, 24).contiguous()
    calls = [lambda: eng.bls_verify(tpk, tb, tsig, dst, offsets=to, rand=rand),
             lambda: eng.pairing_check_rlc(tpk, hq, 1, col_g2=tsig, fixed_g1=neg, rand=rand),
             lambda: eng.pairing_check(g1, g2, 2)]
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    res = _events(calls, reps)
    return dict(n=n, bls_verify=res[0], rlc_prehashed=res[1], pairing_check_k2=res[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--hash-n", default="1024,65536,1048576")
    ap.add_argument("--verify-n", default="1024,16384,262144")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    out = dict(device=eng.device_info(), reps=a.reps, hash=[], verify=[])
    for n in [int(x) for x in a.hash_n.split(",") if x]:
        out["hash"].append(time_hash(eng, n, a.reps))
        print(json.dumps(out["hash"][-1]), flush=True)
    for n in [int(x) for x in a.verify_n.split(",") if x]:
        out["verify"].append(time_verify(eng, n, a.reps))
        print(json.dumps(out["verify"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
