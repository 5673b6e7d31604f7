"""Times hash-to-G1 and the min-sig BLS verifiers on one GPU beside their min-pk twins, in the same process, and writes JSON.
  hash      zkp_hash_to_g1_batch_dev beside zkp_hash_to_g2_batch_dev on the same n messages of 32 bytes, and zkp_hash_to_field_g1_batch_dev
            alone (the share of SHA-256 and the reductions).
  verify    zkp_bls_minsig_verify_batch_dev on n signatures of n keys beside zkp_bls_verify_batch_dev on a min-pk instance of the same n.
            Before any timing both accept their instance and refuse it with one message byte changed.
  samekey   zkp_bls_minsig_verify_samekey_batch_dev on n signatures of ONE key beside zkp_bls_minsig_verify_batch_dev on the same
            signatures with the key repeated n times and the same rand; the two must agree on the instance and on a forgery.
Resident tensors, HIP events, warmed up; the median and the spread (min, max) of --reps runs, the calls alternating rep by rep.
Usage: python tools/time_minsig.py [--reps 5] [--n 1024,16384,262144] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DST_G1 = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"
DST_G2 = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"


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


def _dst(eng, tag):
    import torch
    return torch.frombuffer(bytearray(tag), dtype=torch.uint8).to(torch.device("cuda", eng.device))


def _ok(t):
    return int(t.cpu()[0])


def _warm(calls):
    import torch
    for fn in calls:
        fn()
    torch.cuda.synchronize()


def time_hash(eng, n, reps):
    import numpy as np
    from zkvm_pairings_amd import synthetic
    buf, off = synthetic.splitmix64(0x7A6, 4 * n).view(np.uint8), np.arange(n + 1, dtype=np.uint64) * 32
    tb, to, d1, d2 = _t(eng, buf), _t(eng, off), _dst(eng, DST_G1), _dst(eng, DST_G2)
    calls = [lambda: eng.hash_to_g1(tb, d1, offsets=to), lambda: eng.hash_to_g2(tb, d2, offsets=to), lambda: eng.hash_to_field_g1(tb, d1, offsets=to)]
    _warm(calls)
    res = _events(calls, reps)
    return dict(n=n, hash_to_g1=res[0], hash_to_g2=res[1], hash_to_field_g1=res[2])


def _instance(eng, maker, n, **kw):
    _, pks, msgs, sigs = maker(n, engine=eng, **kw)
    buf, off = eng.pack_messages(msgs)
    bad = buf.copy()
    bad[0] ^= 1                                                             # the first byte of the first message that has one
    return _t(eng, pks), _t(eng, sigs), _t(eng, buf), _t(eng, bad), _t(eng, off)


def time_verify(eng, n, reps):
    from zkvm_pairings_amd import synthetic
    rand = _t(eng, eng.rlc_random(n))
    d1, d2 = _dst(eng, DST_G1), _dst(eng, DST_G2)
    spk, ssig, sb, sbad, so = _instance(eng, synthetic.bls_minsig_instance, n, seed=0xB0C)
    ppk, psig, pb, pbad, po = _instance(eng, synthetic.bls_instance, n, seed=0xB0B)
    assert _ok(eng.bls_minsig_verify(spk, sb, ssig, d1, offsets=so, rand=rand)) == 1, "the min-sig instance does not verify"
    assert _ok(eng.bls_minsig_verify(spk, sbad, ssig, d1, offsets=so, rand=rand)) == 0, "a changed message verifies (min-sig)"
    assert _ok(eng.bls_verify(ppk, pb, psig, d2, offsets=po, rand=rand)) == 1, "the min-pk instance does not verify"
    assert _ok(eng.bls_verify(ppk, pbad, psig, d2, offsets=po, rand=rand)) == 0, "a changed message verifies (min-pk)"
    calls = [lambda: eng.bls_minsig_verify(spk, sb, ssig, d1, offsets=so, rand=rand), lambda: eng.bls_verify(ppk, pb, psig, d2, offsets=po, rand=rand)]
    _warm(calls)
    res = _events(calls, reps)
    return dict(n=n, bls_minsig_verify=res[0], bls_verify=res[1])


def time_samekey(eng, n, reps):
    from zkvm_pairings_amd import synthetic
    rand = _t(eng, eng.rlc_random(n))
    d1 = _dst(eng, DST_G1)
    pk, sig, b, bad, o = _instance(eng, synthetic.bls_minsig_instance, n, same_key=True, seed=0xB0D)
    pk1 = pk[:1].contiguous()
    for msgs, want in ((b, 1), (bad, 0)):
        assert _ok(eng.bls_minsig_verify_samekey(pk1, msgs, sig, d1, offsets=o, rand=rand)) == want, "the same-key verifier: %d wanted" % want
        assert _ok(eng.bls_minsig_verify(pk, msgs, sig, d1, offsets=o, rand=rand)) == want, "the general verifier on the repeated key: %d wanted" % want
    calls = [lambda: eng.bls_minsig_verify_samekey(pk1, b, sig, d1, offsets=o, rand=rand), lambda: eng.bls_minsig_verify(pk, b, sig, d1, offsets=o, rand=rand)]
    _warm(calls)
    res = _events(calls, reps)
    return dict(n=n, bls_minsig_verify_samekey=res[0], bls_minsig_verify_key_repeated=res[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", default="1024,16384,262144")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    out = dict(device=eng.device_info(), reps=a.reps, hash=[], verify=[], samekey=[])
    for n in [int(x) for x in a.n.split(",") if x]:
        for part, fn in (("hash", time_hash), ("verify", time_verify), ("samekey", time_samekey)):
            out[part].append(fn(eng, n, a.reps))
            print(json.dumps({part: out[part][-1]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
