"""The cell recovery on one MI355X where a wrong kernel could pass tests/test_gpu_recover.py (zkp_das_recover_batch, include/zkp_recover.h),
byte for byte, on the host and the device flavour and under both cell orders:
  - every column size M = 2^mu, mu = 1 .. 10, with one cell value, with idle column slots and with two workgroups per blob
    (recover_shapes.EVERY_MU: the round schedules of column_transform, the twiddle-free stage, M = 256 and M = 512);
  - single-coefficient forgeries (tests/recover_forgeries.py): f + a X^(i0 + l t0), whose decoded tails are non-zero at ONE place - one
    element of one lane of one workgroup of k_rec_column must see it - for every column and EVERY tail position, between monomials below N
    that must come back exactly; with erasures on top, where the monomial also wraps, and with exactly M / 2 cells, where it is data;
  - the erasure counts around the lane cuts of k_rec_vanish at M = 1024, and exponents of k_rec_zinv with several bits set;
  - the contracts at the boundary: any non-zero mask byte, outputs prefilled with 0xA5, field values with structure, the wrapper's cell
    indices in any order.
Expected values never come from the library under test: a consistent blob is the coefficients its cells were made from, a blob with too
few cells is zeros, a forged one has ok = 0 and a canonical row, one with exactly M / 2 cells is tests/recover_model.py's interpolant.
Run with -m gpu."""
import ctypes
import random

import numpy as np
import pytest

import poly_model as pm
import recover_forgeries as rf
import recover_model as rm
import recover_replay_cases as rrc
import recover_shapes as rs
from replay_cases import fr_rows

pytestmark = pytest.mark.gpu
R = pm.R
ORDERS = pytest.mark.parametrize("bitrev", [False, True])


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def from_dev(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def both_flavours(eng, inst, log2_n, log2_l, bitrev, what):
    co, ok = eng.das_recover(inst["values"], inst["present"], log2_n, log2_l, bitrev)
    rf.check(co, ok, inst, what + " host")
    dco, dok = eng.das_recover(to_dev(inst["values"]), to_dev(inst["present"]), log2_n, log2_l, bitrev)
    dco, dok = from_dev(dco), from_dev(dok)
    rf.check(dco, dok, inst, what + " dev")
    assert dco.tobytes() == co.tobytes() and dok.tobytes() == ok.tobytes(), what       # the unspecified rows included: the arithmetic is exact
    return co, ok


# ------------------------------------------------------------------------------------------------------------------- A. every column size
@ORDERS
@pytest.mark.parametrize("shape", rs.EVERY_MU, ids=["M%d-l%d" % (1 << s[2], 1 << s[1]) for s in rs.EVERY_MU])
def test_every_column_size(eng, shape, bitrev):
    """three blobs per shape: half the cells at random, the last cell missing, one cell too few"""
    log2_n, log2_l = shape[:2]
    inst = rrc.instance(rs.EVERY_MU_KINDS, log2_n, log2_l, bitrev, 0xE0 + shape[2])
    assert inst["ok"].tolist() == [1, 1, 0] and not inst["free"]
    both_flavours(eng, inst, log2_n, log2_l, bitrev, "M=2^%d l=2^%d" % (shape[2], log2_l))


# ------------------------------------------------------------------------------------------------------------------- B. forgeries
@ORDERS
@pytest.mark.parametrize("log2_n,log2_l,cols", rs.FORGERY_SWEEPS, ids=["N%d-l%d" % (1 << s[0], 1 << s[1]) for s in rs.FORGERY_SWEEPS])
def test_every_single_coefficient_forgery_is_flagged_with_all_cells_present(eng, log2_n, log2_l, cols, bitrev):
    """one call per shape, one monomial per blob: X^(i0 + l t0) for every column i0 (at N = 4096, l = 64: the first and the last column of
    the first workgroup, the first of the second, the last of the blob) and EVERY tail position t0 - ok = 0 -, shuffled among X^e, e < N:
    N - 1, the coefficients the first and the last lane of every workgroup store, one in eight of all - ok = 1 and the unit row exactly.
    X^(N-1) accepted and X^N refused is the boundary of the tail; the good blobs between forged ones keep rows and flags"""
    n, l, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
    inst = rf.sweep(log2_n, log2_l, bitrev, cols)
    assert len(inst["free"]) == (len(cols) if cols else l) * (big_m - k) and {n - 1, n} <= set(inst["exps"].tolist())
    both_flavours(eng, inst, log2_n, log2_l, bitrev, "sweep N=2^%d l=2^%d" % (log2_n, log2_l))


@ORDERS
@pytest.mark.parametrize("how", ["one", "k+1", "k"])
@pytest.mark.parametrize("log2_n,log2_l", rs.FORGERY_ERASED)
def test_single_coefficient_forgeries_under_erasures(eng, log2_n, log2_l, how, bitrev):
    """a random polynomial, a random factor, every (i0, t0).  'one': the last cell missing - every t0 < M - 1 is a single tail element,
    t0 = M - 1 wraps; 'k+1': k + 1 random cells - t0 = k is a single element, every other wraps; both ok = 0.  'k': exactly k cells of the
    same forged data are consistent - ok = 1 and the model's interpolant.  The unforged blob under the same mask in between: ok = 1 and f"""
    inst = rf.erased_sweep(log2_n, log2_l, bitrev, how)
    assert (len(inst["free"]) == 0) == (how == "k") and (inst["ok"].all() == (how == "k")) and inst["ok"].any()
    both_flavours(eng, inst, log2_n, log2_l, bitrev, "%s N=2^%d l=2^%d" % (how, log2_n, log2_l))


# ------------------------------------------------------------------------------------------------------------------- C. the LDS limit
@ORDERS
def test_erasure_counts_at_the_lds_limit(eng, bitrev):
    """M = 1024, one call: 0, 1, 255, 256, 257, 341, 511, 512 and 513 random cells missing, then the first half and the odd cells (the
    sparse Z): f while at most 512 are missing, a zero row and ok = 0 for 513"""
    inst = rf.limit_instance(*rs.LIMIT, rs.LIMIT_MISSING, bitrev)
    assert inst["ok"].tolist() == [1] * 8 + [0, 1, 1]
    co, _ = both_flavours(eng, inst, *rs.LIMIT, bitrev, "limit")
    assert not co.reshape(11, -1)[8].any()


# ------------------------------------------------------------------------------------------------------------------- D. the contracts
@ORDERS
@pytest.mark.parametrize("log2_n,log2_l,kinds", [rs.SMALL + (("few", "random-half", "more-bad", "one", "few", "none", "half-bad"),),
                                                 (10, 2, ("random-half", "few", "one"))], ids=["N16-l4", "N1024-l4"])
def test_any_non_zero_mask_byte_is_a_present_cell(eng, log2_n, log2_l, kinds, bitrev):
    """2, 0x80 and 0xFF mixed with 1: the bytes of the 0 / 1 call, on both flavours (three kernels read the mask, each for itself)"""
    inst = rrc.instance(kinds, log2_n, log2_l, bitrev, 0x3A5)
    other = rf.other_mask_bytes(inst)
    co, ok = both_flavours(eng, inst, log2_n, log2_l, bitrev, "0/1 mask")
    oco, ook = both_flavours(eng, other, log2_n, log2_l, bitrev, "other mask bytes")
    assert oco.tobytes() == co.tobytes() and ook.tobytes() == ok.tobytes()


@ORDERS
def test_every_output_byte_is_written_over_poison(eng, bitrev):
    """out_coeffs and out_ok prefilled with 0xA5 (no canonical element, no flag), through the C ABI: good, too few and forged blobs mixed -
    afterwards every flag is 0 or 1 as stated, every good row is f, every row of too few cells is ALL zero, every forged row canonical"""
    from zkvm_pairings_amd import _lib
    log2_n, log2_l = rs.SMALL
    inst = rf.mixed_instance(log2_n, log2_l, bitrev)
    n, n_co = inst["ok"].size, 1 << log2_n
    flags = _lib.NTT_BITREV if bitrev else 0
    lib, h = eng._lib, eng._h
    poison = lambda: (np.full((n * n_co, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.frombuffer(b"\xa5" * (4 * n), dtype=np.int32).copy())
    co, ok = poison()
    assert not rf.canonical(co[:1]) and ok[0] not in (0, 1)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.zkp_das_recover_batch(h, p(inst["values"]), p(inst["present"]), n, log2_n, log2_l, flags, p(co), p(ok)) == 0
    rf.check(co, ok, inst, "poisoned host")
    few = [j for j in range(n) if inst["labels"][j] == "few"]
    assert len(few) == 3 and not co.reshape(n, -1)[few].any()
    dv, dp, (dco, dok) = to_dev(inst["values"]), to_dev(inst["present"]), [to_dev(a) for a in poison()]
    assert from_dev(dok).tobytes() == b"\xa5" * (4 * n) and from_dev(dco).tobytes() == b"\xa5" * (32 * n * n_co)
    t = lambda x: ctypes.c_void_p(x.data_ptr())
    assert lib.zkp_das_recover_batch_dev(h, t(dv), t(dp), n, log2_n, log2_l, flags, t(dco), t(dok), eng._stream()) == 0
    rf.check(from_dev(dco), from_dev(dok), inst, "poisoned dev")
    assert from_dev(dco).tobytes() == co.tobytes()


@ORDERS
def test_field_values_with_structure(eng, bitrev):
    """f = 0 (ok = 1 and a zero row, beside a blob with too few cells: ok = 0 and a zero row), f constant, every coefficient r - 1,
    X^(N-1), zero cells with exactly k present, and 0, 1, 2, r - 2, r - 1, 2^(32 j) -+ 1 as coefficients, under five patterns each"""
    inst = rf.structured_instance(*rs.SMALL, bitrev)
    assert 0 in inst["ok"] and not inst["free"]
    both_flavours(eng, inst, *rs.SMALL, bitrev, "structured")


@ORDERS
def test_the_wrapper_takes_the_cell_indices_in_any_order(eng, bitrev):
    """recover_polynomials_batch: shuffled indices (the cells shuffled with them) give the bytes of the sorted call, which are f"""
    import zkvm_pairings_amd as z
    log2_n, log2_l = rs.SMALL
    n_co, l, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
    rng = random.Random(0x0DE2 + bitrev)
    idx, cells, want, oks = [], [], [], []
    for keep in (k, big_m, k - 1, k + 1):
        f = [rng.randrange(R) for _ in range(n_co)]
        rows = rm.cells_of(f, log2_n, log2_l, bitrev)
        have = rng.sample(range(big_m), keep)
        assert have != sorted(have)
        idx.append(have)
        cells.append(fr_rows([v for m in have for v in rows[m]]).reshape(keep, l, 4))
        want += f if keep >= k else [0] * n_co
        oks.append(1 if keep >= k else 0)
    co, ok = z.recover_polynomials_batch(idx, cells, log2_n, log2_l, bitrev=bitrev, engine=eng)
    order = [np.argsort(i) for i in idx]
    sco, sok = z.recover_polynomials_batch([np.asarray(i)[o] for i, o in zip(idx, order)], [c[o] for c, o in zip(cells, order)], log2_n, log2_l, bitrev=bitrev,
                                           engine=eng)
    assert ok.tolist() == sok.tolist() == oks and co.tobytes() == sco.tobytes() == fr_rows(want).tobytes()
