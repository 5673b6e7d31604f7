"""The Groth16 producer side on one MI355X (include/zkp_prove.h): the sparse product against Python integers on the shape table of
tests/prove_shapes.py; the quotient against tests/prove_model.py byte for byte; the proofs against [e] g for exponents computed from
the circuit's trapdoor (one oracle multiplication of the generator each) and against the verifier that is already there; slices;
every argument error of the host flavour; a malformed matrix in the device flavour.  Run with -m gpu."""
import ctypes
import random

import numpy as np
import pytest

import prove_model as pmod
import prove_replay_cases as prc
import prove_shapes as ps
from replay_cases import fr_rows

pytestmark = pytest.mark.gpu
R = pmod.R
ERR_ARG, ERR_NONCANONICAL = -1, -4


@pytest.fixture(scope="module")
def eng():
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def helper():
    """the engine the keys are made with: the engine under test sees only the calls under test"""
    from zkvm_pairings_amd import PairingEngine
    e = PairingEngine(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def mat_dev(mat):
    n_rows, n_cols, row_ptr, col, val = mat
    return (n_rows, n_cols, to_dev(row_ptr), to_dev(col), to_dev(val))


# ------------------------------------------------------------------------------------------------------------------- the sparse product
@pytest.mark.parametrize("n", ps.SPMV_N)
@pytest.mark.parametrize("name", list(ps.SPMV))
def test_spmv_equals_python_integers(eng, name, n):
    """host and device flavour, out_stride = n_rows and n_rows + 3; the device flavour writes into a buffer pre-filled with ones, so the
    padding is seen to be written as zero"""
    import torch
    rows, n_cols = ps.spmv_matrix(name)
    xs = ps.spmv_vectors(name, n)
    mat = (len(rows), n_cols) + ps.csr(rows)
    x = fr_rows([v for row in xs for v in row])
    dmat, dx = mat_dev(mat), to_dev(x)
    for out_stride in (len(rows), len(rows) + 3):
        want = ps.spmv_expected(rows, xs, out_stride).tobytes()
        got = eng.fr_spmv(mat, x, out_stride)
        assert got.shape == (n, out_stride, 4) and got.tobytes() == want, (name, n, out_stride, "host")
        keep = []
        rec = eng._csr(dmat, "mat", keep, True)
        out = torch.ones((n, out_stride, 4), dtype=torch.int64, device=dx.device)
        eng._chk(eng._lib.zkp_fr_spmv_batch_dev(eng._h, ctypes.byref(rec), eng._tp(dx), n, out_stride, eng._tp(out), eng._stream()))
        assert out.cpu().numpy().tobytes() == want, (name, n, out_stride, "dev")
        assert eng.fr_spmv(dmat, dx, out_stride).cpu().numpy().tobytes() == want
    assert eng.take_validation_status() is False
    assert ps.expected_t(ps.SPMV[name][0]) in range(7)


# ------------------------------------------------------------------------------------------------------------------- the quotient
@pytest.mark.parametrize("log2_n,n_rows", [(k, r) for k in ps.QUOTIENT_LOG2 for r in ps.quotient_rows(k)])
def test_quotient_equals_the_model(eng, log2_n, n_rows):
    from zkvm_pairings_amd import synthetic
    big_n = 1 << log2_n
    sec = synthetic.groth16_circuit_secrets(0x9007 + 64 * log2_n + n_rows, log2_n, n_rows, big_n + 3, 1, 3, bad=(1,))
    mats = tuple((n_rows, big_n + 3) + synthetic.csr_arrays(sec[x]) for x in ("rows_a", "rows_b", "rows_c"))
    wit = fr_rows([v for z in sec["z"] for v in z])
    model = [pmod.quotient(sec, z) for z in sec["z"]]
    want_h = fr_rows([v for h, _ in model for v in h]).tobytes()
    assert [s for _, s in model] == [True, False, True]
    assert all(h[big_n - 1] == 0 for h, s in model if s)
    h, sat = eng.groth16_quotient(log2_n, 1, *mats, wit)
    assert h.shape == (3, big_n, 4) and h.tobytes() == want_h, (log2_n, n_rows, "host")
    assert sat.tolist() == [1, 0, 1]
    assert not h[0, big_n - 1].any() and not h[2, big_n - 1].any()
    dh, dsat = eng.groth16_quotient(log2_n, 1, *(mat_dev(m) for m in mats), to_dev(wit))
    assert dh.cpu().numpy().tobytes() == want_h and dsat.cpu().numpy().tolist() == [1, 0, 1], (log2_n, n_rows, "dev")


def test_quotient_of_no_rows_and_of_no_witness(eng):
    empty = (0, 5, np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=np.uint64))
    wit = fr_rows([1, 2, 3, 4, 5] * 2)
    h, sat = eng.groth16_quotient(3, 1, empty, empty, empty, wit)
    assert h.shape == (2, 8, 4) and not h.any() and sat.tolist() == [1, 1]
    h, sat = eng.groth16_quotient(3, 1, empty, empty, empty, np.zeros((0, 4), dtype=np.uint64))
    assert h.shape == (0, 8, 4) and sat.shape == (0,)


# ------------------------------------------------------------------------------------------------------------------- the prover
_instances = {}


def instance(helper, log2_n, n_inputs):
    """five witnesses of one circuit (N rows, m = N + 3), witness 1 off by one; kept for the two batch sizes"""
    from zkvm_pairings_amd import synthetic
    key = (log2_n, n_inputs)
    if key not in _instances:
        big_n = 1 << log2_n
        _instances[key] = synthetic.groth16_circuit_instance(0x6A07 + 16 * log2_n + n_inputs, log2_n, big_n, big_n + 3, n_inputs, 5, bad=(1,), engine=helper)
    return _instances[key]


def subset(sec, idx):
    out = dict(sec)
    out["z"] = [sec["z"][j] for j in idx]
    return out


@pytest.mark.parametrize("log2_n,n_inputs,n", ps.PROVER)
def test_proofs_equal_the_exponents_and_verify(eng, helper, log2_n, n_inputs, n):
    import zkvm_pairings_amd as z
    r1cs, pk, vk, wit, sec = instance(helper, log2_n, n_inputs)
    assert pk.a_inf.any() and pk.b_g1_inf.any() and pk.b_g2_inf.any()                 # at least one infinite entry in each query
    assert pk.a_inf[-1] and pk.b_g1_inf[-1] and pk.b_g2_inf[-1] and not pk.l_inf[-1]
    idx = list(range(n))
    bad = [j for j in idx if j == 1]
    sub = subset(sec, idx)
    w = np.ascontiguousarray(wit[:n])
    inputs = np.ascontiguousarray(w[:, 1:n_inputs + 1])
    rng = random.Random(0xB11D + 100 * log2_n + 10 * n_inputs + n)
    for kind in ("random", "zero"):
        rs = [(rng.randrange(R), rng.randrange(R)) if kind == "random" else (0, 0) for _ in idx]
        (ea, eia, eb, eib, ec, eic), esat = prc.expected_proofs(sub, rs)
        rs_rows = fr_rows([v for p in rs for v in p]).reshape(n, 2, 4)
        (a, b, c), (ia, ib, ic), sat = z.groth16_prove_batch(r1cs, pk, w, rs_rows, engine=eng)
        what = (log2_n, n_inputs, n, kind)
        assert sat.tolist() == esat.tolist() == [0 if j in bad else 1 for j in idx], what
        assert (ia.tolist(), ib.tolist(), ic.tolist()) == (eia.tolist(), eib.tolist(), eic.tolist()) and not ia.any() and not ib.any() and not ic.any(), what
        assert a.tobytes() == ea.tobytes(), what + ("A",)
        assert b.tobytes() == eb.tobytes(), what + ("B",)
        assert c.tobytes() == ec.tobytes(), what + ("C",)
        good = [j for j in idx if j not in bad]
        assert z.groth16_verify_batch(vk, (a[good], b[good], c[good]), inputs[good], engine=eng) is True, what
        each = z.groth16_verify_each(vk, (a, b, c), inputs, engine=eng)
        assert each.tolist() == [j not in bad for j in idx], what
        if bad:
            assert z.groth16_verify_batch(vk, (a, b, c), inputs, engine=eng) is False, what
        if kind == "random":       # the device flavour gives the same bytes
            mats = [mat_dev(m) for m in r1cs.matrices()]
            dpk = {name: (None if x is None else to_dev(x)) for name, x in pk.arrays().items()}
            outs = eng.groth16_prove(log2_n, n_inputs, *mats, dpk, to_dev(w.reshape(-1, 4)), to_dev(rs_rows.reshape(-1, 4)))
            host = (a, ia, b, ib, c, ic, sat)
            assert all(t.cpu().numpy().tobytes() == h.tobytes() for t, h in zip(outs, host)), what
    assert eng.take_validation_status() is False


def test_default_blinding_is_fresh_and_the_proofs_verify(eng, helper):
    import zkvm_pairings_amd as z
    r1cs, pk, vk, wit, _ = instance(helper, 2, 1)
    w = np.ascontiguousarray(wit[[0, 2]])
    p1, _, sat1 = z.groth16_prove_batch(r1cs, pk, w, engine=eng)
    p2, _, sat2 = z.groth16_prove_batch(r1cs, pk, w, engine=eng)
    assert sat1.tolist() == sat2.tolist() == [1, 1]
    assert p1[0].tobytes() != p2[0].tobytes()                                         # r and s are drawn per call
    for p in (p1, p2):
        assert z.groth16_verify_batch(vk, p, w[:, 1:2], engine=eng) is True


def test_slices(eng, helper):
    """more proofs than one slice holds: the whole batch verifies, and the first and the last proof of every slice equal their exponents"""
    import zkvm_pairings_amd as z
    from zkvm_pairings_amd import synthetic
    log2_n, m, n = ps.SLICES["log2_n"], ps.SLICES["m"], ps.SLICES["n"]
    per = max(1, (1 << 22) // max(m, 1 << log2_n))                                    # the header's slice formula
    starts = list(range(0, n, per))
    assert len(starts) >= 2 and n % per != 0                                          # several slices and a short last one
    base = 7
    r1cs, pk, vk, wit, sec = synthetic.groth16_circuit_instance(0x511CE, log2_n, 1 << log2_n, m, 1, base, engine=helper)
    which = [j % base for j in range(n)]
    w = np.ascontiguousarray(wit[which])
    rng = random.Random(0x511CE)
    rs = [(rng.randrange(R), rng.randrange(R)) for _ in range(n)]
    (a, b, c), (ia, ib, ic), sat = z.groth16_prove_batch(r1cs, pk, w, fr_rows([v for p in rs for v in p]).reshape(n, 2, 4), engine=eng)
    assert sat.all() and not ia.any() and not ib.any() and not ic.any()
    assert z.groth16_verify_batch(vk, (a, b, c), np.ascontiguousarray(w[:, 1:2]), engine=eng) is True
    edge = sorted(set(starts + [s - 1 for s in starts[1:]] + [n - 1]))
    (ea, _, eb, _, ec, _), _ = prc.expected_proofs(subset(sec, [which[j] for j in edge]), [rs[j] for j in edge])
    assert a[edge].tobytes() == ea.tobytes() and b[edge].tobytes() == eb.tobytes() and c[edge].tobytes() == ec.tobytes(), edge


# ------------------------------------------------------------------------------------------------------------------- errors
class Args:
    """a valid host call on a small circuit, as ctypes records one can spoil field by field"""

    def __init__(self, r1cs, pk, wit, n):
        from zkvm_pairings_amd import _lib
        self.keep = []
        self.n, self.m = n, r1cs.m
        self.rec = _lib.R1cs(log2_n=r1cs.log2_n, n_inputs=r1cs.n_inputs)
        for name, (row_ptr, col, val) in zip("abc", (r1cs.a, r1cs.b, r1cs.c)):
            arrs = [row_ptr.copy(), col.copy(), val.copy()]
            self.keep += arrs
            setattr(self.rec, name, _lib.FrCsr(n_rows=r1cs.n_rows, n_cols=r1cs.m, nnz=col.size, row_ptr=arrs[0].ctypes.data, col=arrs[1].ctypes.data,
                                               val=arrs[2].ctypes.data))
        self.key = _lib.Groth16Pk()
        for name, x in pk.arrays().items():
            if x is not None and x.size:
                self.keep.append(x)
                setattr(self.key, name, x.ctypes.data)
        self.wit = wit[:n].copy()                        # the tests write into it: never the instance's own array
        self.rs = np.zeros((n, 8), dtype=np.uint64)
        self.h = np.zeros((n, 1 << r1cs.log2_n, 4), dtype=np.uint64)
        self.pa, self.pb, self.pc = (np.zeros((n, w), dtype=np.uint64) for w in (12, 24, 12))
        self.ia, self.ib, self.ic, self.sat = (np.zeros(n, dtype=np.uint8) for _ in range(4))

    def quotient(self, eng, n=None, wit=True, out=True):
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        return eng._lib.zkp_groth16_quotient_batch(eng._h, ctypes.byref(self.rec), p(self.wit) if wit else None, self.n if n is None else n,
                                                   p(self.h) if out else None, p(self.sat))

    def prove(self, eng, flags=0, rs=True):
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        return eng._lib.zkp_groth16_prove_batch(eng._h, ctypes.byref(self.rec), ctypes.byref(self.key), p(self.wit), p(self.rs) if rs else None, self.n, flags,
                                                p(self.pa), p(self.ia), p(self.pb), p(self.ib), p(self.pc), p(self.ic), p(self.sat))

    def spmv(self, eng, n=None, out_stride=None, x=True):
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        return eng._lib.zkp_fr_spmv_batch(eng._h, ctypes.byref(self.rec.a), p(self.wit) if x else None, self.n if n is None else n,
                                          self.rec.a.n_rows if out_stride is None else out_stride, p(self.h))


def test_argument_errors_of_the_host_flavour(eng, helper):
    r1cs, pk, _, wit, _ = instance(helper, 2, 1)                   # N = 4, four rows, m = 7
    fresh = lambda: Args(r1cs, pk, wit, 2)
    a = fresh()
    assert a.quotient(eng) == 0 and a.prove(eng) == 0 and a.spmv(eng) == 0 and a.sat.tolist() == [1, 0]
    assert a.quotient(eng, n=0, wit=False, out=False) == 0         # n == 0 is legal
    cases = {
        "log2_n 0": lambda a: setattr(a.rec, "log2_n", 0),
        "log2_n 21": lambda a: setattr(a.rec, "log2_n", 21),
        "n_rows > N": lambda a: [setattr(m, "n_rows", 5) for m in (a.rec.a, a.rec.b, a.rec.c)],
        "rows disagree": lambda a: setattr(a.rec.b, "n_rows", 3),
        "columns disagree": lambda a: setattr(a.rec.c, "n_cols", 8),
        "n_inputs + 1 > m": lambda a: setattr(a.rec, "n_inputs", 7),
        "m > 2^22": lambda a: [setattr(m, "n_cols", (1 << 22) + 1) for m in (a.rec.a, a.rec.b, a.rec.c)],
        "nnz > 2^31 - 1": lambda a: setattr(a.rec.a, "nnz", 1 << 31),
        "null row_ptr": lambda a: setattr(a.rec.a, "row_ptr", None),
        "null col": lambda a: setattr(a.rec.b, "col", None),
        "null val": lambda a: setattr(a.rec.c, "val", None),
    }
    for what, spoil in cases.items():
        a = fresh()
        spoil(a)
        assert a.quotient(eng) == ERR_ARG and a.prove(eng) == ERR_ARG, what
    a = fresh()
    assert a.quotient(eng, wit=False) == ERR_ARG and a.quotient(eng, out=False) == ERR_ARG and a.prove(eng, rs=False) == ERR_ARG
    assert a.prove(eng, flags=1) == ERR_ARG and a.prove(eng, flags=-1) == ERR_ARG                      # unknown flags
    for field in ("alpha_g1", "delta_g2", "a_query", "b_g2_query", "l_query", "h_query"):
        a = fresh()
        setattr(a.key, field, None)
        assert a.prove(eng) == ERR_ARG, field
    # the product's own limits
    a = fresh()
    assert a.spmv(eng, out_stride=3) == ERR_ARG and a.spmv(eng, out_stride=(1 << 20) + 1) == ERR_ARG and a.spmv(eng, x=False) == ERR_ARG
    assert a.spmv(eng, n=(1 << 26) // 4 + 1) == ERR_ARG and a.spmv(eng, n=0, x=False) == 0
    # a malformed matrix in host memory
    spoils = {
        "row_ptr[0] != 0": lambda m, rp, col: rp.__setitem__(0, 1),
        "not monotone": lambda m, rp, col: rp.__setitem__(2, int(rp[1]) - 1) if rp[1] else rp.__setitem__(1, int(rp[2]) + 1),
        "row_ptr[n_rows] != nnz": lambda m, rp, col: rp.__setitem__(4, int(rp[4]) - 1),
        "col >= n_cols": lambda m, rp, col: col.__setitem__(0, 7),
    }
    for what, spoil in spoils.items():
        a = fresh()
        spoil(a.rec.a, a.keep[0], a.keep[1])
        assert a.spmv(eng) == ERR_ARG and a.quotient(eng) == ERR_ARG and a.prove(eng) == ERR_ARG, what
    assert fresh().quotient(eng) == 0


def test_noncanonical_inputs_in_validation_mode(helper):
    from zkvm_pairings_amd import PairingEngine
    r1cs, pk, _, wit, _ = instance(helper, 2, 1)
    e = PairingEngine(0, validate=True)
    try:
        a = Args(r1cs, pk, wit, 2)
        assert a.quotient(e) == 0 and a.prove(e) == 0
        r_row = fr_rows([R])[0]
        a.keep[2][0] = r_row                                      # a value of A
        assert a.quotient(e) == ERR_NONCANONICAL and a.prove(e) == ERR_NONCANONICAL and a.spmv(e) == ERR_NONCANONICAL
        a = Args(r1cs, pk, wit, 2)
        a.wit[1, 3] = r_row
        assert a.quotient(e) == ERR_NONCANONICAL and a.prove(e) == ERR_NONCANONICAL and a.spmv(e) == ERR_NONCANONICAL
        a = Args(r1cs, pk, wit, 2)
        a.rs[1, 4:] = r_row
        assert a.quotient(e) == 0 and a.prove(e) == ERR_NONCANONICAL
        # the device flavour ORs into the validation word
        mats = [mat_dev(m) for m in r1cs.matrices()]
        w = np.ascontiguousarray(wit[:2]).reshape(-1, 4)
        e.groth16_quotient(2, 1, *mats, to_dev(w))
        assert e.take_validation_status() is False
        w[3] = r_row
        e.groth16_quotient(2, 1, *mats, to_dev(w))
        assert e.take_validation_status() is True
    finally:
        e.close()


def test_malformed_matrix_in_the_device_flavour_sets_the_validation_word(eng):
    """the kernel's guards were shown under ASan on host threads (test_prove_cpu.py) before this runs on a GPU: a column >= n_cols and
    row bounds beyond nnz contribute nothing, the call returns normally, the word is set - with validation mode off"""
    rows, n_cols = ps.spmv_matrix("len7")
    rows = rows[:20]
    xs = ps.spmv_vectors("len7", 3)
    rp, cl, val = ps.csr(rows)
    nnz = int(rp[-1])
    x = to_dev(fr_rows([v for row in xs for v in row]))
    assert eng.take_validation_status() is False
    col = cl.copy()
    col[3], col[50] = n_cols, 0xFFFFFFFF
    kept = [[(c, v) for i, (c, v) in enumerate(row) if 7 * k + i not in (3, 50)] for k, row in enumerate(rows)]
    out = eng.fr_spmv((20, n_cols, to_dev(rp), to_dev(col), to_dev(val)), x)
    assert out.cpu().numpy().tobytes() == ps.spmv_expected(kept, xs, 20).tobytes()
    assert eng.take_validation_status() is True and eng.take_validation_status() is False
    bad = rp.copy()
    bad[10], bad[20] = nnz + 5, 0xFFFFFFF0
    lo = [min(int(bad[k]), nnz) for k in range(20)]
    hi = [min(int(bad[k + 1]), nnz) for k in range(20)]
    flat = [e for row in rows for e in row]
    kept = [flat[min(lo[k], hi[k]):hi[k]] for k in range(20)]
    out = eng.fr_spmv((20, n_cols, to_dev(bad), to_dev(cl), to_dev(val)), x)
    assert out.cpu().numpy().tobytes() == ps.spmv_expected(kept, xs, 20).tobytes()
    assert eng.take_validation_status() is True
    out = eng.fr_spmv((20, n_cols, to_dev(rp), to_dev(cl), to_dev(val)), x)
    assert out.cpu().numpy().tobytes() == ps.spmv_expected(rows, xs, 20).tobytes() and eng.take_validation_status() is False


def test_plain_c_consumer_of_the_third_header(tmp_path):
    """integration/c/zkp_prove.c: the descriptors and two of the calls from plain C (no Python, no torch types)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "zkp_prove")
    libdir = os.path.join(root, "zkvm_pairings_amd")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "integration", "c", "zkp_prove.c"),
                           "-L", libdir, "-lzkp_pairings", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "zkp_prove ok: A z = (3, 1), sat = (1, 0)" in out.stdout
