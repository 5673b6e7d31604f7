"""The device-pointer entry points of include/zkp_bls_minsig.h captured into a hipGraph and replayed on changed inputs, by the protocol
of tests/test_gpu_graph_replay.py (imported, not copied): the eager call, the capture, five replays on the sets A, A, B, C, A with
sentinels in the outputs, a smaller eager call, a sixth replay.  The cases and their expected bytes: tests/minsig_replay_cases.py.
And the call order: large / 1 / large / small min-sig calls on ONE context between bls_verify and hash_to_g2, which share the RLC and MSM
workspaces with the min-sig verifiers (the hash workspaces are separate): every answer must be what the call gives alone.  Run with -m gpu."""
import numpy as np
import pytest

import bls_replay_cases as brc
import h2c_model as h
import h2g1_model as g
import minsig_pools as mp
import minsig_replay_cases as mrc
from test_gpu_graph_replay import replay_protocol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", mrc.CASES, ids=[c.id for c in mrc.CASES])
def test_captured_minsig_calls_replay_on_changed_inputs(eng, helper, case):
    replay_protocol(eng, helper, case)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.copy()).cuda()


def test_large_one_large_small_between_bls_verify_and_hash_to_g2():
    """on a fresh context: hash_to_g1 on 2^17 + 61 messages, bls_verify on 61, hash_to_g1 on 1, the min-sig verifier on 1, hash_to_g2 on 5,
    the same-key verifier on 2^17 + 61 signatures (valid, then forged behind the slice boundary), bls_verify on 5 (valid, swapped), the
    min-sig verifier on 61 (valid, swapped), hash_to_g1 on 2^17 + 61 again, both min-sig verifiers on 5, bls_verify on 61"""
    import torch
    from zkvm_pairings_amd import PairingEngine
    idx = mp.index_sequence()
    n_big = idx.size
    buf, off = mp.packed(idx)
    pool = mp.pool_messages()
    want_pool, winf_pool = mrc.point_rows([mrc.hashed(x, mrc.DST) for x in pool])
    sk, pk = mrc.signed_pool()[0][0], mrc.signed_pool()[0][1]
    sig_pool = mrc.u64([g.g1_words(mrc.rc._cached(("minsig-same", x), lambda x=x: g.e_mul(mrc.hashed(x, mrc.DST), sk)))[0] for x in pool]).reshape(-1, 12)
    pk1 = mrc.u64(h.g2_words(pk)[0]).reshape(1, 24)
    few = [b"", b"one", bytes(range(56)), b"\x00" * 64, bytes(range(119, 0, -1))]
    want_g2, winf_g2 = brc.point_rows([brc.hashed(x, brc.DST) for x in few])
    pk_small, pk_big = brc.batch(5, 3), brc.batch(61, 4)
    ms_one, ms_small, ms_big = mrc.batch(1, 2), mrc.batch(5, 3), mrc.batch(61, 4)
    same_small = mrc.same_key_batch(5, 3)
    e = PairingEngine(0)
    try:
        d_buf, d_off = _dev(buf), _dev(off)

        def big_hash(step):
            pts, inf = e.hash_to_g1(d_buf, mrc.DST, offsets=d_off)
            torch.cuda.synchronize()
            pts, inf = pts.cpu().numpy().view(np.uint64), inf.cpu().numpy()
            assert pts.tobytes() == want_pool[idx].tobytes() and inf.tobytes() == winf_pool[idx].tobytes(), step

        def minpk(b, want, step, swap=False):
            sig = b["sig"][[1, 0] + list(range(2, len(b["msgs"])))] if swap else b["sig"]
            assert e.bls_verify(b["pk"], b["msgs"], sig, brc.DST, rand=brc.rand_rows(len(b["msgs"]), 9)) is want, step

        def minsig(b, want, step, swap=False):
            sig = b["sig"][[1, 0] + list(range(2, len(b["msgs"])))] if swap else b["sig"]
            assert e.bls_minsig_verify(b["pk"], b["msgs"], sig, mrc.DST, rand=mrc.rand_rows(len(b["msgs"]), 9)) is want, step

        big_hash(0)
        minpk(pk_big, True, 1)
        one, one_inf = e.hash_to_g1([pool[7]], mrc.DST)
        assert one.tobytes() == want_pool[7:8].tobytes() and not one_inf.any(), 2
        minsig(ms_one, True, 3)
        pts, inf = e.hash_to_g2(few, brc.DST)
        assert pts.tobytes() == want_g2.tobytes() and inf.tobytes() == winf_g2.tobytes(), 4
        d_pk, d_rand = _dev(pk1), _dev(mrc.rand_rows(n_big, 11))
        for forged in (None, mp.SLICE + 3):
            sig = sig_pool[idx]
            if forged is not None:
                sig[forged] = sig[forged - 1] if idx[forged] != idx[forged - 1] else sig_pool[(idx[forged] + 1) % mp.POOL]
            ok = e.bls_minsig_verify_samekey(d_pk, d_buf, _dev(sig), mrc.DST, offsets=d_off, rand=d_rand, points_checked=True)
            torch.cuda.synchronize()
            assert bool(ok.item()) is (forged is None), (5, forged)
        minpk(pk_small, True, 6)
        minpk(pk_small, False, 6, swap=True)
        minsig(ms_big, True, 7)
        minsig(ms_big, False, 7, swap=True)
        big_hash(8)
        minsig(ms_small, True, 9)
        assert e.bls_minsig_verify_samekey(same_small["pk1"], same_small["msgs"], same_small["sig"], mrc.DST, rand=mrc.rand_rows(5, 9)) is True, 9
        assert e.bls_minsig_verify(same_small["pk"], same_small["msgs"], same_small["sig"], mrc.DST, rand=mrc.rand_rows(5, 9)) is True, 9
        minpk(pk_big, True, 10)
        pts, inf = e.hash_to_g2(few, brc.DST)
        assert pts.tobytes() == want_g2.tobytes() and inf.tobytes() == winf_g2.tobytes(), 11
    finally:
        e.close()
