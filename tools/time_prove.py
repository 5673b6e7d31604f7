"""Times the Groth16 producer side on one GPU and writes JSON, per stage and against the floors nothing removes:
  spmv     zkp_fr_spmv_batch_dev on the A matrix of the circuit (n witnesses) against the same number of products, nnz n, through
           zkp_fr_op_batch_dev(ZKP_FR_MUL) - the only Fr product the library offered before, and without the gathers or the sums;
  quotient zkp_groth16_quotient_batch_dev (three products, seven NTTs, the pointwise kernels);
  msm      each of the prover's five shared-bases MSM calls alone through zkp_g*_msm_batch_dev: a_query, b_g1_query, b_g2_query and
           l_query over the witness rows, h_query over the h rows;
  prove    zkp_groth16_prove_batch_dev against the SUM of those five MSM calls - the floor: the prover cannot beat its own MSMs.
The circuit is synthetic.groth16_circuit_instance (N rows, m = N + 3, one public input); the witnesses are a few distinct ones tiled
to n, all satisfying (sat must be all ones, and the batch must verify).  Resident tensors, HIP events, warmed up; the median of --reps
runs, the alternatives alternating.
Usage: python tools/time_prove.py [--reps R] [--logs 10,14] [--n 64] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = 4


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
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(torch.device("cuda", eng.device))


def _row(eng, log2_n, n, reps, warmup):
    import numpy as np
    import torch
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import synthetic
    big_n, m = 1 << log2_n, (1 << log2_n) + 3
    r1cs, pk, vk, wit, _ = synthetic.groth16_circuit_instance(0x71AE + log2_n, log2_n, big_n, m, 1, BASE, engine=eng)
    w = np.ascontiguousarray(wit[[j % BASE for j in range(n)]])
    rs = eng.fr_from_wide(np.frombuffer(os.urandom(n * 2 * 64), dtype=np.uint8))
    mats = [(mt[0], mt[1], _t(eng, mt[2]), _t(eng, mt[3]), _t(eng, mt[4])) for mt in r1cs.matrices()]
    dpk = {name: (None if x is None else _t(eng, x)) for name, x in pk.arrays().items()}
    dw, drs = _t(eng, w.reshape(-1, 4)), _t(eng, rs)
    nnz = int(r1cs.a[1].size)
    # the same number of products through fr_op: nnz n pairs of elements
    fa = _t(eng, synthetic.scalars(1, min(nnz * n, 1 << 20)))
    fa = fa.repeat((nnz * n + fa.shape[0] - 1) // fa.shape[0], 1)[:nnz * n].contiguous()
    # the padded queries of the L and H sums, as the prover builds them
    l_pad = torch.zeros((m, 12), dtype=torch.int64, device=dw.device)
    l_pad[2:] = dpk["l_query"]
    l_inf = torch.ones(m, dtype=torch.uint8, device=dw.device)
    l_inf[2:] = dpk["l_inf"]
    h_pad = torch.zeros((big_n, 12), dtype=torch.int64, device=dw.device)
    h_pad[:big_n - 1] = dpk["h_query"]
    h_inf = torch.zeros(big_n, dtype=torch.uint8, device=dw.device)
    h_inf[big_n - 1] = 1
    h, sat = eng.groth16_quotient(log2_n, 1, *mats, dw)
    assert bool(sat.all())
    calls = {
        "spmv": lambda: eng.fr_spmv(mats[0], dw, big_n),
        "fr_op_mul_same_products": lambda: eng.fr_op("mul", fa, fa),
        "quotient": lambda: eng.groth16_quotient(log2_n, 1, *mats, dw),
        "msm_a": lambda: eng.g1_msm(dpk["a_query"], dw, n, dpk["a_inf"], shared_bases=True),
        "msm_b_g1": lambda: eng.g1_msm(dpk["b_g1_query"], dw, n, dpk["b_g1_inf"], shared_bases=True),
        "msm_b_g2": lambda: eng.g2_msm(dpk["b_g2_query"], dw, n, dpk["b_g2_inf"], shared_bases=True),
        "msm_l": lambda: eng.g1_msm(l_pad, dw, n, l_inf, shared_bases=True),
        "msm_h": lambda: eng.g1_msm(h_pad, h.reshape(-1, 4), n, h_inf, shared_bases=True),
        "prove": lambda: eng.groth16_prove(log2_n, 1, *mats, dpk, dw, drs),
    }
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    pa, ia, pb, ib, pc, ic, psat = calls["prove"]()
    proofs = tuple(t.cpu().numpy().view(np.uint64) for t in (pa, pb, pc))
    assert bool(psat.all()) and z.groth16_verify_batch(vk, proofs, np.ascontiguousarray(w[:, 1:2]), engine=eng)
    ms = dict(zip(calls, _events(list(calls.values()), reps)))
    floor = sum(ms[k] for k in ("msm_a", "msm_b_g1", "msm_b_g2", "msm_l", "msm_h"))
    row = {"log2_n": log2_n, "m": m, "n": n, "nnz_a": nnz}
    row.update({k + "_ms": round(v, 4) for k, v in ms.items()})
    row.update({"msm_sum_ms": round(floor, 4), "prove_over_msm_sum": round(ms["prove"] / floor, 3),
                "fr_op_over_spmv": round(ms["fr_op_mul_same_products"] / ms["spmv"], 3)})
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--logs", default="10,14")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from zkvm_pairings_amd import PairingEngine
    eng = PairingEngine(0)
    rows = [_row(eng, int(k), a.n, a.reps, a.warmup) for k in a.logs.split(",")]
    res = {"tool": "time_prove", "device": eng.device_info(), "reps": a.reps, "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
