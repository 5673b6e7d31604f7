"""Times the G2 segment sums, the min-sig FastAggregateVerify and AggregateVerify on one GPU and writes JSON.  Every baseline is composed
of calls the library had before include/zkp_bls_agg_g2.h, in the same run:
  check     before any timing: the sums of the first shape equal the add tree's, the instances verify, and one changed entry makes them
            fail.
  sum       zkp_g2_segment_sum_batch_dev over a table of --table G2 points, segments x size as in --shapes, beside a torch gather of the
            members followed by a tree of zkp_g2_add_batch_dev calls (log2(size) launches, an inversion per addition; uniform
            power-of-two segments only).
  verify    zkp_bls_minsig_fast_aggregate_verify_batch_dev at the shapes of --verify-shapes beside zkp_bls_minsig_verify_batch_dev on the
            precomputed aggregates: the difference is what the sums add.
  aggregate zkp_bls_aggregate_verify_batch_dev at the shapes of --aggregate-shapes (signatures x messages per signature) beside
            zkp_bls_verify_batch_dev on arrays expanded outside the timing: the difference is what the expansion adds.
Resident tensors, HIP events, warmed up; the median and the spread (min, max) of --reps runs, the calls alternating rep by rep.
Usage: python tools/time_agg_g2.py [--reps R] [--table 1048576] [--shapes 16384x64,2048x512,1x1048576] [--verify-shapes 16384x64,2048x512]
                                   [--aggregate-shapes 16384x64,2048x512,1x1048576] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
MINSIG_DST = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_POP_"


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


def _shapes(text):
    return [tuple(int(v) for v in x.split("x")) for x in text.split(",") if x]


def _ints(sks):
    w = sks.astype(object)
    return list(w[:, 0] + (w[:, 1] << 64) + (w[:, 2] << 128) + (w[:, 3] << 192))


def _table(eng, n_table):
    """(secret keys as Python integers, the resident table): pk_i = [sk_i] g2 on the engine"""
    from zkvm_pairings_amd import synthetic
    sks = synthetic.scalars(0xA67, n_table)
    pks, _ = eng.g2_mul(synthetic.G2_GENERATOR, sks)
    return _ints(sks), _t(eng, pks)


def _members(n_table, count, size, seed):
    """count x size table rows from the seed (with repetition across segments, which a sum does not mind)"""
    import numpy as np
    from zkvm_pairings_amd import synthetic
    return (synthetic.splitmix64(seed, count * size) % np.uint64(n_table)).astype(np.uint32).reshape(count, size)


def _add_tree(eng, table, rows):
    """the members gathered, then halved by pairwise additions until one point per segment is left"""
    pts = table[rows.reshape(-1).long()].reshape(rows.shape[0], rows.shape[1], 24)
    inf = None
    while pts.shape[1] > 1:
        half = pts.shape[1] // 2
        a, b = pts[:, :half].reshape(-1, 24).contiguous(), pts[:, half:].reshape(-1, 24).contiguous()
        ia, ib = (None, None) if inf is None else (inf[:, :half].reshape(-1).contiguous(), inf[:, half:].reshape(-1).contiguous())
        out, oi = eng.g2_add(a, b, ia, ib)
        pts, inf = out.reshape(rows.shape[0], half, 24), oi.reshape(rows.shape[0], half)
    return pts.reshape(-1, 24), inf


def time_sum(eng, table, n_table, count, size, reps, check):
    import numpy as np
    import torch
    rows = _members(n_table, count, size, 0xC0118 + size)
    idx, seg_off = _t(eng, rows.reshape(-1)), _t(eng, np.arange(count + 1, dtype=np.uint64) * size)
    trows = _t(eng, rows)
    tree = size & (size - 1) == 0 and count * size <= 1 << 24
    out, inf, st = eng.g2_segment_sum(table, idx, seg_off)                # also grows the workspace
    assert not bool(st.any()) and not bool(inf.any()), "a random segment summed to the identity or was refused"
    if tree and check:
        want, _ = _add_tree(eng, table, trows)
        assert torch.equal(out, want), "segment sums differ from the add tree"
    calls = [lambda: eng.g2_segment_sum(table, idx, seg_off)] + ([lambda: _add_tree(eng, table, trows)] if tree else [])
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    res = _events(calls, reps)
    return dict(segments=count, size=size, segment_sum=res[0], gather_add_tree=res[1] if tree else None)


def time_verify(eng, sks, table, n_table, count, size, reps):
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    rows = _members(n_table, count, size, 0xFA58 + size)
    sums = np.stack([synthetic.int_to_scalar(sum(sks[r] for r in c) % synthetic.R_ORDER) for c in rows.tolist()])
    msgs = synthetic.splitmix64(0x5E5B, 4 * count).view(np.uint8)
    off = np.arange(count + 1, dtype=np.uint64) * 32
    h, _ = eng.hash_to_g1(msgs, MINSIG_DST, offsets=off)
    sigs, _ = eng.g1_mul(h, sums)
    idx, seg_off = _t(eng, rows.reshape(-1)), _t(eng, np.arange(count + 1, dtype=np.uint64) * size)
    tsig, tb, to, rand = _t(eng, sigs), _t(eng, msgs), _t(eng, off), _t(eng, eng.rlc_random(count))
    dst = torch.frombuffer(bytearray(MINSIG_DST), dtype=torch.uint8).to(table.device)
    assert int(eng.bls_minsig_fast_aggregate_verify(table, idx, seg_off, tb, tsig, dst, offsets=to, rand=rand).cpu()[0]) == 1, "the instance does not verify"
    bad = idx.clone()
    bad[-1] = (int(rows[-1, -1]) + 1) % n_table
    assert int(eng.bls_minsig_fast_aggregate_verify(table, bad, seg_off, tb, tsig, dst, offsets=to, rand=rand).cpu()[0]) == 0, "a changed committee verifies"
    apk, ainf, _ = eng.g2_segment_sum(table, idx, seg_off)
    calls = [lambda: eng.bls_minsig_fast_aggregate_verify(table, idx, seg_off, tb, tsig, dst, offsets=to, rand=rand),
             lambda: eng.bls_minsig_verify(apk, tb, tsig, dst, offsets=to, inf_pk=ainf, rand=rand)]
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    res = _events(calls, reps)
    return dict(committees=count, size=size, minsig_fast_aggregate_verify=res[0], minsig_verify_on_precomputed_aggregates=res[1])


def time_aggregate(eng, count, size, reps):
    """count signatures over size (key, message) pairs each: the individual signatures are made and summed on the engine"""
    import numpy as np
    import torch
    from zkvm_pairings_amd import synthetic
    n_msg = count * size
    sks = synthetic.scalars(0xA6B + size, n_msg)
    pks, _ = eng.g1_mul(synthetic.G1_GENERATOR, sks)
    msgs = synthetic.splitmix64(0x5E5C + size, 4 * n_msg).view(np.uint8)
    off = np.arange(n_msg + 1, dtype=np.uint64) * 32
    h, _ = eng.hash_to_g2(msgs, DST, offsets=off)
    each, _ = eng.g2_mul(h, sks)
    seg = np.arange(count + 1, dtype=np.uint64) * size
    dev = torch.device("cuda", eng.device)
    seg_off = _t(eng, seg)
    sig, sinf, _ = eng.g2_segment_sum(_t(eng, each), torch.arange(n_msg, dtype=torch.int32, device=dev), seg_off)
    assert not bool(sinf.any())
    tpk, tb, to, rand = _t(eng, pks), _t(eng, msgs), _t(eng, off), _t(eng, eng.rlc_random(count))
    dst = torch.frombuffer(bytearray(DST), dtype=torch.uint8).to(dev)
    # the expansion, outside the timing: the signature under the first message of its segment, the flagged identity elsewhere
    first = torch.arange(count, device=dev) * size
    x_sig = torch.zeros((n_msg, 24), dtype=torch.int64, device=dev)
    x_sig[:, 12] = 1
    x_sig[first] = sig
    x_inf = torch.ones(n_msg, dtype=torch.uint8, device=dev)
    x_inf[first] = 0
    x_rand = rand.repeat_interleave(size, dim=0).contiguous()
    assert int(eng.bls_aggregate_verify(tpk, tb, seg_off, sig, dst, offsets=to, rand=rand).cpu()[0]) == 1, "the instance does not verify"
    assert int(eng.bls_verify(tpk, tb, x_sig, dst, offsets=to, inf_sig=x_inf, rand=x_rand).cpu()[0]) == 1, "the expanded instance does not verify"
    bad = tpk.clone()
    bad[[0, n_msg - 1]] = bad[[n_msg - 1, 0]]
    assert int(eng.bls_aggregate_verify(bad, tb, seg_off, sig, dst, offsets=to, rand=rand).cpu()[0]) == 0, "two swapped keys verify"
    calls = [lambda: eng.bls_aggregate_verify(tpk, tb, seg_off, sig, dst, offsets=to, rand=rand),
             lambda: eng.bls_verify(tpk, tb, x_sig, dst, offsets=to, inf_sig=x_inf, rand=x_rand)]
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    res = _events(calls, reps)
    return dict(signatures=count, size=size, aggregate_verify=res[0], bls_verify_on_expanded_arrays=res[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--table", type=int, default=1 << 20)
    ap.add_argument("--shapes", default="16384x64,2048x512,1x1048576")
    ap.add_argument("--verify-shapes", default="16384x64,2048x512")
    ap.add_argument("--aggregate-shapes", default="16384x64,2048x512,1x1048576")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    sks, table = _table(eng, a.table)
    out = dict(device=eng.device_info(), reps=a.reps, table=a.table, sum=[], verify=[], aggregate=[])
    for i, (count, size) in enumerate(_shapes(a.shapes)):
        out["sum"].append(time_sum(eng, table, a.table, count, size, a.reps, check=i == 0))
        print(json.dumps(out["sum"][-1]), flush=True)
    for count, size in _shapes(a.verify_shapes):
        out["verify"].append(time_verify(eng, sks, table, a.table, count, size, a.reps))
        print(json.dumps(out["verify"][-1]), flush=True)
    del table
    for count, size in _shapes(a.aggregate_shapes):
        out["aggregate"].append(time_aggregate(eng, count, size, a.reps))
        print(json.dumps(out["aggregate"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
