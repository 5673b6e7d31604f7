"""Times BLS verification grouped by message on one GPU and writes JSON.
  verify     zkp_bls_verify_grouped_batch_dev on --n signatures over each count of --messages distinct messages (equal groups), beside the
             baseline zkp_bls_verify_batch_dev on the same signatures with the messages expanded, in the same process on the same inputs.
             Before any timing both must accept the instance and refuse it with two signatures swapped.
  aggregate  zkp_bls_fast_aggregate_verify_grouped_batch_dev at the shapes of --committee (committees x size x messages) beside
             zkp_bls_fast_aggregate_verify_batch_dev on the expanded messages, over a table of --table keys.
  sum        zkp_g1_scaled_segment_sum_batch_dev alone beside zkp_g1_mul_endo_batch_dev followed by zkp_g1_segment_sum_batch_dev on the same
             points and scalars (the scaled points as the table, every row once); the two must give the same bytes.
Resident tensors, HIP events, warmed up; the median and the spread (min, max) of --reps runs, the calls alternating rep by rep.
Usage: python tools/time_grouped.py [--reps R] [--n 16384] [--messages 16384,256,1] [--committee 16384x64x256] [--table 1048576] [--out FILE]"""
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
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(torch.device("cuda", eng.device))


def _messages(count, seed):
    """count distinct messages of 32 bytes: (bytes (count, 32), offsets)"""
    import numpy as np
    from zkvm_pairings_amd import synthetic
    raw = synthetic.splitmix64(seed, 4 * count).reshape(count, 4)
    raw[:, 0] = np.arange(count, dtype=np.uint64)                        # the message's number leads: pairwise distinct
    return raw.view(np.uint8).reshape(count, 32), np.arange(count + 1, dtype=np.uint64) * 32


def _groups(n, m):
    """group of each of n items in m equal groups (ordered), and the m + 1 offsets"""
    import numpy as np
    grp = (np.arange(n, dtype=np.int64) * m) // n
    off = np.zeros(m + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(grp, minlength=m)).astype(np.uint64)
    return grp, off


def _warm(calls):
    import torch
    for fn in calls:
        fn()
    torch.cuda.synchronize()


def time_verify(eng, n, m, reps):
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    sks = synthetic.scalars(0x6B15 + m, n)
    pks, _ = eng.g1_mul(synthetic.G1_GENERATOR, sks)
    msgs, off = _messages(m, 0x65E5)
    grp, grp_off = _groups(n, m)
    h, _ = eng.hash_to_g2(msgs.reshape(-1), DST, offsets=off)
    sigs, _ = eng.g2_mul(h[grp], sks)
    dev = torch.device("cuda", eng.device)
    dst = torch.frombuffer(bytearray(DST), dtype=torch.uint8).to(dev)
    pk, sig, rand = _t(eng, pks), _t(eng, sigs), _t(eng, eng.rlc_random(n))
    tg, tb, to = _t(eng, grp_off), _t(eng, msgs.reshape(-1)), _t(eng, off)
    eb, eo = _t(eng, msgs[grp].reshape(-1)), _t(eng, np.arange(n + 1, dtype=np.uint64) * 32)
    grouped = lambda s=sig: eng.bls_verify_grouped(pk, tg, tb, s, dst, offsets=to, rand=rand)
    flat = lambda s=sig: eng.bls_verify(pk, eb, s, dst, offsets=eo, rand=rand)
    assert int(grouped().cpu()[0]) == 1 and int(flat().cpu()[0]) == 1, "the instance does not verify"
    if n > 1:
        bad = sig.clone()
        bad[[0, n - 1]] = sig[[n - 1, 0]]
        assert int(grouped(bad).cpu()[0]) == 0 and int(flat(bad).cpu()[0]) == 0, "two swapped signatures verify"
    calls = [grouped, flat]
    _warm(calls)
    res = _events(calls, reps)
    return dict(signatures=n, messages=m, bls_verify_grouped=res[0], bls_verify_expanded=res[1])


def time_sum(eng, n, m, reps):
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    pks, _ = eng.g1_mul(synthetic.G1_GENERATOR, synthetic.scalars(0x5CA1 + m, n))
    _, seg_off = _groups(n, m)
    pts, rand, off = _t(eng, pks), _t(eng, eng.rlc_random(n)), _t(eng, seg_off)
    rows = _t(eng, np.arange(n, dtype=np.uint32))

    def two_calls():
        scaled, _ = eng.g1_mul_endo(pts, rand)
        return eng.g1_segment_sum(scaled, rows, off)
    one = lambda: eng.g1_scaled_segment_sum(pts, rand, off)
    a, b = one(), two_calls()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the scaled segment sums differ from mul_endo + segment_sum"
    calls = [one, two_calls]
    _warm(calls)
    res = _events(calls, reps)
    return dict(points=n, segments=m, g1_scaled_segment_sum=res[0], mul_endo_then_segment_sum=res[1])


def time_aggregate(eng, n_table, count, size, m, reps):
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    sks = synthetic.scalars(0xA66, n_table)
    table, _ = eng.g1_mul(synthetic.G1_GENERATOR, sks)
    w = sks.astype(object)
    ints = list(w[:, 0] + (w[:, 1] << 64) + (w[:, 2] << 128) + (w[:, 3] << 192))
    rows = (synthetic.splitmix64(0xFA57 + size, count * size) % np.uint64(n_table)).astype(np.uint32).reshape(count, size)
    sums = np.stack([synthetic.int_to_scalar(sum(ints[r] for r in c) % synthetic.R_ORDER) for c in rows.tolist()])
    msgs, off = _messages(m, 0x5E5A)
    grp, grp_off = _groups(count, m)
    h, _ = eng.hash_to_g2(msgs.reshape(-1), DST, offsets=off)
    sigs, _ = eng.g2_mul(h[grp], sums)
    dev = torch.device("cuda", eng.device)
    dst = torch.frombuffer(bytearray(DST), dtype=torch.uint8).to(dev)
    tt, idx, seg_off = _t(eng, table), _t(eng, rows.reshape(-1)), _t(eng, np.arange(count + 1, dtype=np.uint64) * size)
    sig, rand = _t(eng, sigs), _t(eng, eng.rlc_random(count))
    tg, tb, to = _t(eng, grp_off), _t(eng, msgs.reshape(-1)), _t(eng, off)
    eb, eo = _t(eng, msgs[grp].reshape(-1)), _t(eng, np.arange(count + 1, dtype=np.uint64) * 32)
    grouped = lambda i=idx: eng.bls_fast_aggregate_verify_grouped(tt, i, seg_off, tg, tb, sig, dst, offsets=to, rand=rand)
    flat = lambda i=idx: eng.bls_fast_aggregate_verify(tt, i, seg_off, eb, sig, dst, offsets=eo, rand=rand)
    assert int(grouped().cpu()[0]) == 1 and int(flat().cpu()[0]) == 1, "the instance does not verify"
    bad = idx.clone()
    bad[-1] = (int(rows[-1, -1]) + 1) % n_table
    assert int(grouped(bad).cpu()[0]) == 0 and int(flat(bad).cpu()[0]) == 0, "a changed committee verifies"
    calls = [grouped, flat]
    _warm(calls)
    res = _events(calls, reps)
    return dict(committees=count, size=size, messages=m, fast_aggregate_verify_grouped=res[0], fast_aggregate_verify_expanded=res[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 14)
    ap.add_argument("--messages", default="16384,256,1")
    ap.add_argument("--committee", default="16384x64x256")
    ap.add_argument("--table", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    out = dict(device=eng.device_info(), reps=a.reps, verify=[], sum=[], aggregate=[])
    for m in [int(v) for v in a.messages.split(",") if v]:
        out["verify"].append(time_verify(eng, a.n, min(m, a.n), a.reps))
        print(json.dumps(out["verify"][-1]), flush=True)
        out["sum"].append(time_sum(eng, a.n, min(m, a.n), a.reps))
        print(json.dumps(out["sum"][-1]), flush=True)
    for count, size, m in [tuple(int(v) for v in x.split("x")) for x in a.committee.split(",") if x]:
        out["aggregate"].append(time_aggregate(eng, a.table, count, size, m, a.reps))
        print(json.dumps(out["aggregate"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
