"""The minimal-signature-size BLS verifiers on one MI355X (run with -m gpu): batches signed by tests/h2g1_model.py (signatures in G1,
public keys in G2), the batch verifier, the same-key verifier and the per-signature path on valid, forged and malformed batches."""
import ctypes
import functools

import numpy as np
import pytest

import bls12_381_model as m
import h2c_model as h
import h2g1_model as g
import minsig_pools as mp
import outside_groups as og

pytestmark = pytest.mark.gpu
DST = g.QUICKNET_DST
POOL = 8


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def u64(rows):
    return np.array(rows, dtype=np.uint64)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


@functools.lru_cache(maxsize=None)
def signed_pool():
    """POOL tuples (sk, pk in G2, msg, sig in G1) from the model; entry 0 and entry 1 share messages of length 0 and 1"""
    out = []
    for i in range(POOL):
        sk = 0x1234567 * (i + 1) + (0xABCDEF << (20 * i))
        msg = bytes((11 * i + j) & 0xFF for j in range(i * 9 % 70))
        out.append((sk, g.sk_to_pk(sk), msg, g.sign(sk, msg, DST)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def same_key_pool():
    """the key of entry 0 on the 64 messages of tests/minsig_pools.py: (pk, [sig of pool message j])"""
    sk = signed_pool()[0][0]
    return signed_pool()[0][1], tuple(g.sign(sk, x, DST) for x in mp.pool_messages())


def batch(n):
    pool = signed_pool()
    idx = [(3 * i + n) % POOL for i in range(n)]
    return dict(idx=idx, pk=u64([h.g2_words(pool[k][1])[0] for k in idx]).reshape(n, 24), msgs=[pool[k][2] for k in idx],
                sig=u64([g.g1_words(pool[k][3])[0] for k in idx]).reshape(n, 12))


def rand_rows(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 1 << 63, size=(n, 2), dtype=np.uint64)


def verify_both(eng, b, want_all, want_each=None, msgs=None, **kw):
    """the batch verifier on host arrays and on resident tensors, and the per-signature path"""
    import torch
    import zkvm_pairings_amd as z
    msgs = b["msgs"] if msgs is None else msgs
    n = len(msgs)
    rand = kw.pop("rand", None)
    rand = rand_rows(n, 7) if rand is None else rand
    assert eng.bls_minsig_verify(b["pk"], msgs, b["sig"], DST, rand=rand, **kw) is want_all
    buf, off = eng.pack_messages(msgs)
    dkw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    ok = eng.bls_minsig_verify(dev(b["pk"]), dev(buf) if buf.size else None, dev(b["sig"]), DST, offsets=dev(off), rand=dev(rand), **dkw)
    torch.cuda.synchronize()
    assert bool(ok.item()) is want_all
    each = z.bls_minsig_verify_each(b["pk"], msgs, b["sig"], DST, engine=eng, **kw)
    assert each.tolist() == list(np.full(n, want_all) if want_each is None else want_each)


def _down(n, *where):
    each = np.ones(n, dtype=bool)
    each[list(where)] = False
    return each


def _flags(n, *where):
    f = np.zeros(n, dtype=np.uint8)
    f[list(where)] = 1
    return f


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_valid_batches_and_one_forged_signature_at_the_first_middle_and_last_position(eng, n):
    b = batch(n)
    verify_both(eng, b, True)
    other = g.g1_words(g.e_mul(m.G1_GEN, 0xF00D))[0]
    for j in sorted({0, n // 2, n - 1}):
        bad = dict(b, sig=b["sig"].copy())
        bad["sig"][j] = u64(other)
        verify_both(eng, bad, False, _down(n, j))


@pytest.mark.parametrize("n", [5, 65])
def test_swapped_messages_identity_keys_and_identity_signatures(eng, n):
    b = batch(n)
    msgs = list(b["msgs"])
    msgs[0], msgs[1] = msgs[1], msgs[0]
    verify_both(eng, b, False, _down(n, 0, 1), msgs=msgs)
    for j in (0, n // 2, n - 1):
        verify_both(eng, b, False, _down(n, j), inf_pk=_flags(n, j))
        verify_both(eng, b, False, _down(n, j), inf_pk=_flags(n, j), points_checked=True)       # KeyValidate is no part of the skipped check
        verify_both(eng, b, False, _down(n, j), inf_sig=_flags(n, j))
    verify_both(eng, b, True, points_checked=True)


@pytest.mark.parametrize("n", [5, 65])
def test_keys_off_the_curve_or_outside_g2_and_signatures_outside_g1(eng, n):
    b = batch(n)
    pool = signed_pool()
    g2_bad = [q for q in og.g2_points().values() if not m.g2_on_curve(q)][:1] + [q for q in og.g2_points().values() if m.g2_on_curve(q) and not m.g2_torsion_free(q)][:2]
    assert len(g2_bad) == 3
    for k, j in enumerate((0, n // 2, n - 1)):
        bad = dict(b, pk=b["pk"].copy())
        bad["pk"][j] = u64(h.g2_words(g2_bad[k])[0])
        verify_both(eng, bad, False, _down(n, j))
        # sig + T, T of order 3 or 11: the pairing equation still holds, only the subgroup check refuses the signature
        sig = pool[b["idx"][j]][3]
        shifted = m.g1_add(sig, og.g1_points()[("order3", "order11", "order3_neg")[k]])
        assert m.g1_on_curve(shifted) and not m.g1_torsion_free(shifted)
        bad = dict(b, sig=b["sig"].copy())
        bad["sig"][j] = u64(g.g1_words(shifted)[0])
        verify_both(eng, bad, False, _down(n, j))
        off = (sig[0], (sig[1] + 1) % g.P)
        bad["sig"][j] = u64(g.g1_words(off)[0])
        verify_both(eng, bad, False, _down(n, j))


@pytest.mark.parametrize("n", [5, 65])
def test_a_zero_row_of_rand_fails_the_batch_and_half_zero_rows_do_not(eng, n):
    """the rule of tests/test_gpu_bls.py: (0, 0) would drop a check from the product; (a, 0) and (0, b) are non-zero exponents"""
    b = batch(n)
    for j in (0, n // 2, n - 1):
        rand = rand_rows(n, 31 + j)
        rand[j] = 0
        verify_both(eng, b, False, np.ones(n, dtype=bool), rand=rand)
    rand = rand_rows(n, 35)
    rand[0, 1] = 0
    rand[n // 2, 0] = 0
    rand[n - 1, 1] = 0
    verify_both(eng, b, True, rand=rand)


def _samekey(n, idx=None):
    pk, sigs = same_key_pool()
    idx = [(5 * i + 1) % mp.POOL for i in range(n)] if idx is None else idx
    pool = mp.pool_messages()
    return dict(pk1=u64(h.g2_words(pk)[0]).reshape(1, 24), pk=np.tile(u64(h.g2_words(pk)[0]), (n, 1)), msgs=[pool[k] for k in idx],
                sig=u64([g.g1_words(sigs[k])[0] for k in idx]).reshape(n, 12))


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_same_key_verifier_equals_the_general_one_with_the_key_repeated(eng, n):
    import torch
    b = _samekey(n)
    rand = rand_rows(n, 41)
    other = u64(g.g1_words(g.e_mul(m.G1_GEN, 0xBEEF))[0])
    for forged in (None, 0, n // 2, n - 1):
        sig = b["sig"].copy()
        if forged is not None:
            sig[forged] = other
        want = forged is None
        assert eng.bls_minsig_verify(b["pk"], b["msgs"], sig, DST, rand=rand) is want
        assert eng.bls_minsig_verify_samekey(b["pk1"], b["msgs"], sig, DST, rand=rand) is want
        buf, off = eng.pack_messages(b["msgs"])
        ok = eng.bls_minsig_verify_samekey(dev(b["pk1"]), dev(buf) if buf.size else None, dev(sig), DST, offsets=dev(off), rand=dev(rand))
        torch.cuda.synchronize()
        assert bool(ok.item()) is want
    assert eng.bls_minsig_verify_samekey(b["pk1"], b["msgs"], b["sig"], DST, rand=rand, inf_sig=_flags(n, n - 1)) is False
    zero = rand.copy()
    zero[n // 2] = 0
    assert eng.bls_minsig_verify_samekey(b["pk1"], b["msgs"], b["sig"], DST, rand=zero) is False


def test_same_key_verifier_refuses_the_identity_and_keys_outside_g2(eng):
    b = _samekey(5)
    identity = u64(h.g2_words(None)[0]).reshape(1, 24)
    for checked in (False, True):
        assert eng.bls_minsig_verify_samekey(identity, b["msgs"], b["sig"], DST, points_checked=checked) is False
    for q in og.g2_points().values():
        assert eng.bls_minsig_verify_samekey(u64(h.g2_words(q)[0]).reshape(1, 24), b["msgs"], b["sig"], DST) is False
    assert eng.bls_minsig_verify_samekey(b["pk1"], b["msgs"], b["sig"], DST, points_checked=True) is True


def test_same_key_verifier_across_the_slice_boundary(eng):
    """2^17 + 61 signatures of one key over the pool's messages: valid, then one forgery on either side of the boundary"""
    import torch
    idx = mp.index_sequence()
    n = idx.size
    pk, sigs = same_key_pool()
    rows = u64([g.g1_words(s)[0] for s in sigs]).reshape(mp.POOL, 12)
    buf, off = mp.packed(idx)
    d_pk, d_buf, d_off, d_rand = dev(u64(h.g2_words(pk)[0]).reshape(1, 24)), dev(buf), dev(off), dev(rand_rows(n, 43))
    other = u64(g.g1_words(g.e_mul(m.G1_GEN, 0xBEEF))[0])
    for forged in (None, mp.SLICE - 1, mp.SLICE):
        sig = rows[idx]
        if forged is not None:
            sig[forged] = other
        ok = eng.bls_minsig_verify_samekey(d_pk, d_buf, dev(sig), DST, offsets=d_off, rand=d_rand, points_checked=True)
        torch.cuda.synchronize()
        assert bool(ok.item()) is (forged is None)


def test_cross_variant_pairing_identity_sign_round_trip_and_compressed_inputs(eng):
    import zkvm_pairings_amd as z
    pool = signed_pool()[:5]
    sks = u64([[(sk >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for sk, _, _, _ in pool])
    msgs = [x[2] for x in pool]
    sig, inf = z.bls_minsig_sign_batch(sks, msgs, DST, engine=eng)
    assert sig.tobytes() == u64([g.g1_words(x[3])[0] for x in pool]).tobytes() and not inf.any()
    pk, pinf = z.bls_minsig_keygen_batch(sks, engine=eng)
    assert pk.tobytes() == u64([h.g2_words(x[1])[0] for x in pool]).tobytes() and not pinf.any()
    # e([sk] H(m), g2) == e(H(m), [sk] g2), through pairing_check: (sig, -g2), (H, pk)
    hp, _ = z.hash_to_g1(msgs, DST, engine=eng)
    neg_g2 = u64(h.g2_words(m.g2_neg(m.G2_GEN))[0])
    g1 = np.stack([sig, hp], axis=1).reshape(-1, 12)
    g2 = np.stack([np.tile(neg_g2, (5, 1)), pk], axis=1).reshape(-1, 24)
    per, _ = eng.pairing_check(g1, g2, 2)
    assert np.asarray(per).reshape(-1).tolist() == [1] * 5
    pkb, sgb = eng.compress_points(pk, 2), eng.compress_points(sig, 1)
    assert z.bls_minsig_verify_batch_compressed(pkb, msgs, sgb, DST, engine=eng) is True
    assert z.bls_minsig_verify_each_compressed(pkb, msgs, sgb, DST, engine=eng).tolist() == [True] * 5
    assert z.bls_minsig_verify_batch_compressed(pkb, msgs[1:] + msgs[:1], sgb, DST, engine=eng) is False
    _, pks2, msgs2, sigs2 = z.synthetic.bls_minsig_instance(7, engine=eng)
    assert z.bls_minsig_verify_batch(pks2, msgs2, sigs2, DST, engine=eng) is True
    _, pks3, msgs3, sigs3 = z.synthetic.bls_minsig_instance(7, same_key=True, engine=eng)
    assert z.bls_minsig_verify_samekey_batch(pks3[:1], msgs3, sigs3, DST, engine=eng) is True
    assert z.bls_minsig_verify_batch(pks3, msgs3, sigs3, DST, engine=eng) is True


def test_the_empty_batch_and_the_argument_errors(eng):
    import zkvm_pairings_amd as z
    none24, none12 = np.zeros((0, 24), dtype=np.uint64), np.zeros((0, 12), dtype=np.uint64)
    assert z.bls_minsig_verify_batch(none24, [], none12, DST, engine=eng) is True
    b = _samekey(3)
    assert z.bls_minsig_verify_samekey_batch(b["pk1"], [], none12, DST, engine=eng) is True
    buf, off = eng.pack_messages(b["msgs"])
    rand = rand_rows(3, 5)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    ok = ctypes.c_int(5)
    lib, hd = eng._lib, eng._h
    d = np.frombuffer(DST, dtype=np.uint8)
    long_dst = np.zeros(256, dtype=np.uint8)
    general = lambda dst, dst_len, n, flags, out: lib.zkp_bls_minsig_verify_batch(hd, p(b["pk"]), None, p(buf), p(off), p(dst), dst_len, p(b["sig"]), None, n, p(rand),
                                                                                  flags, out)
    same = lambda pk, dst_len, n, flags, out: lib.zkp_bls_minsig_verify_samekey_batch(hd, pk, p(buf), p(off), p(d), dst_len, p(b["sig"]), None, n, p(rand), flags, out)
    assert general(d, d.size, 3, 0, ctypes.byref(ok)) == 0 and ok.value == 1
    assert general(d, d.size, 3, 2, ctypes.byref(ok)) == -1                  # an unknown flag
    assert general(long_dst, 256, 3, 0, ctypes.byref(ok)) == -1 and general(d, 0, 3, 0, ctypes.byref(ok)) == -1
    assert general(d, d.size, (1 << 24) + 1, 0, ctypes.byref(ok)) == -1 and general(d, d.size, 3, 0, None) == -1
    assert same(p(b["pk1"]), d.size, 3, 0, ctypes.byref(ok)) == 0 and ok.value == 1
    assert same(None, d.size, 3, 0, ctypes.byref(ok)) == -1 and same(None, d.size, 0, 0, ctypes.byref(ok)) == -1
    assert same(p(b["pk1"]), d.size, 3, 4, ctypes.byref(ok)) == -1 and same(p(b["pk1"]), d.size, (1 << 24) + 1, 0, ctypes.byref(ok)) == -1


def test_c_consumer(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "zkvm_pairings_amd")
    exe = str(tmp_path / "zkp_bls_minsig")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, "integration", "c", "zkp_bls_minsig.c"), "-L", libdir,
                           "-lzkp_pairings", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("zkp_bls_minsig ok"), (out.returncode, out.stdout, out.stderr)
