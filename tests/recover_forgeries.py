"""Single-coefficient forgeries and the other instances of test_gpu_recover_forgeries.py and of its CPU twin in test_recover_cpu.py (helper;
not a test module).  f'(X) = f(X) + a X^e with deg f < N, a != 0, e = i0 + l t0 and M / 2 = k <= t0 < M, cut into cells as
recover_model.cells_of cuts f: the monomial lands in column i0 of the decode alone.  With k + s cells present (deg Z = k - s):
  s = 0            any data is consistent: ok = 1 and the row is the other interpolant
  k <= t0 < k + s  the decoded tail is non-zero at ONE place, column i0, position t0, and the low part is f: one element of one lane of one
                   workgroup of k_rec_column sees the inconsistency
  t0 >= k + s      the monomial wraps around into the s tail positions below k + s of column i0, the other columns clean; ok = 0 still
test_recover_cpu.py holds the model (tests/recover_model.py) to these three.  The cells of a bare monomial X^e are w_D^(e pos): rows of
the domain table, gathered by index arithmetic - no transform per blob.  Instances have the form of recover_replay_cases.instance:
dict(values (n M l, 4), present (n M,), coeffs (n N, 4), ok (n,) int32, free: the blobs whose row is unspecified).  Expected values never
come from the library under test."""
import random

import numpy as np

import poly_model as pm
import recover_model as rm
import recover_replay_cases as rrc
import replay_cases as rc
from replay_cases import fr_rows

R = pm.R
TPB, TILE_LOG2 = 256, 10          # k_rec_column: 256 lanes, a tile of 2^10 elements, lane q holds tile elements q, q + 256, q + 512, q + 768
R_WORDS = [(R >> (64 * i)) & rc.M64 for i in range(4)]
# 0, 1, 2, r - 2, r - 1 and 2^(32 j) -+ 1 (mod r), j = 1 .. 7: carries and borrows at every word boundary of the 32-bit kernels
STRUCTURED = [0, 1, 2, R - 2, R - 1] + [((1 << (32 * j)) + d) % R for j in range(1, 8) for d in (-1, 1)]
MASK_BYTES = (1, 2, 0x80, 0xFF)   # present[j][m] != 0 means received


def canonical(rows):
    """every (.., 4) uint64 row is below r (recover_replay_cases.below_r without a Python loop; test_recover_cpu.py compares the two)"""
    a = np.asarray(rows, dtype=np.uint64).reshape(-1, 4)
    lt, eq = np.zeros(len(a), dtype=bool), np.ones(len(a), dtype=bool)
    for i in (3, 2, 1, 0):
        w = np.uint64(R_WORDS[i])
        lt |= eq & (a[:, i] < w)
        eq &= a[:, i] == w
    return bool(lt.all())


def check(got_coeffs, got_ok, inst, what=""):
    """recover_replay_cases.check for batches of a thousand blobs: flags all, rows byte for byte but for the unspecified ones, which must
    be canonical"""
    co, ok = np.asarray(got_coeffs), np.asarray(got_ok)
    n = inst["ok"].size
    assert ok.dtype == np.int32 and ok.shape == (n,), (what, ok.dtype, ok.shape)
    wrong = np.nonzero(ok != inst["ok"])[0]
    assert wrong.size == 0, "%s: %d flags of %d differ, the first at blob %d (%s): %d" % (what, wrong.size, n, wrong[0], label(inst, wrong[0]), ok[wrong[0]])
    co, want = co.reshape(n, -1), inst["coeffs"].reshape(n, -1)
    assert co.shape == want.shape and co.dtype == want.dtype == np.uint64, (what, co.shape, want.shape)
    free = np.zeros(n, dtype=bool)
    free[inst["free"]] = True
    assert canonical(co[free]), what
    wrong = np.nonzero((co != want).any(axis=1) & ~free)[0]
    assert wrong.size == 0, "%s: %d rows of %d differ, the first at blob %d (%s)" % (what, wrong.size, n, wrong[0], label(inst, wrong[0]))
    assert co[~free].tobytes() == want[~free].tobytes()


def label(inst, j):
    return inst["labels"][j] if "labels" in inst else "-"


# ------------------------------------------------------------------------------------------------------------------- monomials by gathering
def domain_table(log2_d):
    """w_D^x, x < D, as (D, 4) uint64"""
    return rc._cached(("forgery-domain", log2_d), lambda: fr_rows(pm.domain(log2_d)))


def positions(log2_n, log2_l, bitrev):
    """(M, l): value u of cell m is f(w_D^pos[m][u]) - recover_model.cells_of's cut of the extended blob: under bitrev the rows of the
    bit-reversed transform, otherwise entry m + M u of the natural-order one"""
    _, l, _, d, big_m, _ = rm.sizes(log2_n, log2_l)
    m, u = np.meshgrid(np.arange(big_m, dtype=np.int64), np.arange(l, dtype=np.int64), indexing="ij")
    if not bitrev:
        return m + big_m * u
    at, out = l * m + u, np.zeros((big_m, l), dtype=np.int64)
    for b in range(log2_n + 1):
        out |= ((at >> b) & 1) << (log2_n - b)
    return out


def monomial_cells(exps, log2_n, log2_l, bitrev):
    """the cells of X^e for every e of exps: (len(exps), M, l, 4)"""
    pos = positions(log2_n, log2_l, bitrev)
    e = np.asarray(exps, dtype=np.int64).reshape(-1, 1, 1)
    return domain_table(log2_n + 1)[(e * pos[None]) & ((2 << log2_n) - 1)]


def tail_exps(log2_n, log2_l, cols=None):
    """(i0, t0, e = i0 + l t0) for the columns i0 (all when cols is None) and EVERY tail position k <= t0 < M"""
    _, l, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
    return [(i0, t0, i0 + l * t0) for i0 in (range(l) if cols is None else cols) for t0 in range(k, big_m)]


def edge_lane_exps(log2_n, log2_l):
    """the coefficients that lane 0 and lane 255 of every workgroup of k_rec_column store: tile element e = q + 256 u holds column slot
    c = e mod 2^cl and position p = e >> cl of workgroup g, which is coefficient g C + c + l bitrev_mu(p) when c < C and bitrev_mu(p) < k
    (C = min(l, 2^cl) columns per workgroup, cl = 10 - mu)"""
    _, l, k, _, _, mu = rm.sizes(log2_n, log2_l)
    cl = TILE_LOG2 - mu
    cols = min(l, 1 << cl)
    out = set()
    for g in range(l // cols):
        for q in (0, TPB - 1):
            for u in range(4):
                e = q + TPB * u
                c, t = e & ((1 << cl) - 1), pm.bit_reverse(e >> cl, mu)
                if c < cols and t < k:
                    out.add(g * cols + c + l * t)
    return sorted(out)


def twin_exps(log2_n, log2_l):
    """the exponents below N of the positive twins: N - 1 (with X^N among the forgeries: the boundary of the tail), 0, the coefficients of
    the edge lanes, and one in eight of all - 8 j + (5 j mod 8), so that the residues mod l move through the columns"""
    n = 1 << log2_n
    return sorted({0, n - 1} | set(edge_lane_exps(log2_n, log2_l)) | {8 * j + 5 * j % 8 for j in range(n // 8)})


def sweep(log2_n, log2_l, bitrev, cols=None):
    """all cells present, one monomial per blob, factor 1 on a zero base: X^e for every (i0, t0) of tail_exps - ok = 0, the row
    unspecified - and for every e of twin_exps - ok = 1 and the unit row exactly -, shuffled, so that good blobs stand between forged ones"""
    def build():
        n_co, _, _, _, big_m, _ = rm.sizes(log2_n, log2_l)
        exps = [(e, "forged i0=%d t0=%d" % (i0, t0)) for i0, t0, e in tail_exps(log2_n, log2_l, cols)] + [(e, "twin e=%d" % e) for e in twin_exps(log2_n, log2_l)]
        random.Random(0xF0 + 32 * log2_n + 2 * log2_l + bitrev).shuffle(exps)
        n = len(exps)
        e = np.array([x[0] for x in exps], dtype=np.int64)
        coeffs = np.zeros((n, n_co, 4), dtype=np.uint64)
        good = np.nonzero(e < n_co)[0]
        coeffs[good, e[good], 0] = 1
        return dict(values=monomial_cells(e, log2_n, log2_l, bitrev).reshape(-1, 4), present=np.ones(n * big_m, dtype=np.uint8), coeffs=coeffs.reshape(-1, 4),
                    ok=(e < n_co).astype(np.int32), free=np.nonzero(e >= n_co)[0].tolist(), labels=[x[1] for x in exps], exps=e)
    if (len(tail_exps(log2_n, log2_l, cols)) << (log2_n + 6)) >= 1 << 26:      # 64 MiB and more, used by one test each: not kept
        return build()
    return rc._cached(("forgery-sweep", log2_n, log2_l, bitrev, cols), build)


# ------------------------------------------------------------------------------------------------------------------- on Python integers
def monomial_rows(e, log2_n, log2_l, bitrev):
    dom, pos = pm.domain(log2_n + 1), positions(log2_n, log2_l, bitrev).tolist()
    return [[dom[e * p % len(dom)] for p in row] for row in pos]


def forge(cells, a, e, log2_n, log2_l, bitrev):
    """the cells of f + a X^e from the cells of f"""
    return [[(v + a * x) % R for v, x in zip(row, mono)] for row, mono in zip(cells, monomial_rows(e, log2_n, log2_l, bitrev))]


def pack(blobs, log2_n, labels=None):
    """(rows or None where missing, present, expected coefficients or None, ok) per blob -> an instance; missing cells hold garbage"""
    rng = random.Random(len(blobs) + log2_n)
    n_co = 1 << log2_n
    vals, pres, co, oks, free = [], [], [], [], []
    for j, (rows, present, want, ok) in enumerate(blobs):
        for row, p in zip(rows, present):
            vals += row if p else rrc.garbage(rng, len(rows[0]))
        pres += present
        if want is None:
            free.append(j)
            want = [0] * n_co
        co += want
        oks.append(ok)
    inst = dict(values=fr_rows(vals), present=np.array(pres, dtype=np.uint8), coeffs=fr_rows(co), ok=np.array(oks, dtype=np.int32), free=free)
    if labels:
        inst["labels"] = list(labels)
    return inst


def keep_cells(big_m, keep, rng):
    kept = set(rng.sample(range(big_m), keep))
    return [1 if m in kept else 0 for m in range(big_m)]


def erased_sweep(log2_n, log2_l, bitrev, how):
    """a random f, a random factor, every (i0, t0) of tail_exps, and erasures on top.  how:
      'one'      the last cell missing (s = k - 1): t0 < M - 1 is a single tail element, t0 = M - 1 wraps; ok = 0
      'k+1'      k + 1 random cells per blob (s = 1): t0 = k is a single tail element, t0 > k wraps; ok = 0
      'k'        exactly k random cells of the same forged data: ok = 1 and the row is recover_model.recover's
    with the unforged f under the same mask after every eighth forgery: ok = 1 and f"""
    def build():
        rng = random.Random(0xE5 + 64 * log2_n + 4 * log2_l + 2 * bitrev + len(how))
        n_co, _, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
        f = [rng.randrange(R) for _ in range(n_co)]
        cells = rm.cells_of(f, log2_n, log2_l, bitrev)
        blobs, labels = [], []
        for j, (i0, t0, e) in enumerate(tail_exps(log2_n, log2_l)):
            present = rm.pattern("one", big_m) if how == "one" else keep_cells(big_m, k + 1 if how == "k+1" else k, rng)
            bad = forge(cells, 1 + rng.randrange(R - 1), e, log2_n, log2_l, bitrev)
            want, ok = (None, 0) if how != "k" else rm.recover(bad, present, log2_n, log2_l, bitrev)
            assert how != "k" or (ok == 1 and want != f)
            blobs.append((bad, present, want, ok))
            labels.append("%s forged i0=%d t0=%d" % (how, i0, t0))
            if j % 8 == 7:
                blobs.append((cells, present, f, 1))
                labels.append("%s unforged" % how)
        return pack(blobs, log2_n, labels)
    return rc._cached(("forgery-erased", log2_n, log2_l, bitrev, how), build)


# ------------------------------------------------------------------------------------------------------------------- the LDS limit
def limit_instance(log2_n, log2_l, missing, bitrev):
    """one blob per count of `missing` with that many random cells gone, then 'first-half' and 'odd' (M / 2 missing: the sparse Z under
    bitrev and in natural order).  f comes back while at most M / 2 cells are missing; one more is a zero row and ok = 0"""
    def build():
        rng = random.Random(0x11D + bitrev)
        n_co, _, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
        blobs, labels = [], []
        for gone in list(missing) + ["first-half", "odd"]:
            f = [rng.randrange(R) for _ in range(n_co)]
            present = rm.pattern(gone, big_m) if isinstance(gone, str) else keep_cells(big_m, big_m - gone, rng)
            few = sum(present) < k
            blobs.append((rm.cells_of(f, log2_n, log2_l, bitrev), present, [0] * n_co if few else f, 0 if few else 1))
            labels.append("%s missing" % gone)
        return pack(blobs, log2_n, labels)
    return rc._cached(("forgery-limit", log2_n, log2_l, tuple(missing), bitrev), build)


# ------------------------------------------------------------------------------------------------------------------- the contracts
def other_mask_bytes(inst):
    """the same instance with 2, 0x80 and 0xFF mixed with 1 where a cell is present"""
    pres = inst["present"].copy()
    at = np.nonzero(pres)[0]
    pres[at] = np.array(MASK_BYTES, dtype=np.uint8)[(at * 7 + at // 5) % len(MASK_BYTES)]
    assert ((pres != 0) == (inst["present"] != 0)).all() and all((pres == b).any() for b in MASK_BYTES)
    return dict(inst, present=pres)


def mixed_instance(log2_n, log2_l, bitrev):
    """good, too few and forged blobs in one batch: every byte of every row and flag is specified but the forged rows, which are canonical"""
    def build():
        rng = random.Random(0xA5 + 8 * log2_n + log2_l + bitrev)
        n_co, l, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
        blobs, labels = [], []
        for kind in ("few", "random-half", "forged", "few", "none", "forged-one", "one", "few"):
            if kind.startswith("forged"):
                f = [rng.randrange(R) for _ in range(n_co)]
                cells = forge(rm.cells_of(f, log2_n, log2_l, bitrev), 1 + rng.randrange(R - 1), rng.randrange(l) + l * k, log2_n, log2_l, bitrev)
                blobs.append((cells, rm.pattern("one" if kind == "forged-one" else "none", big_m), None, 0))
            else:
                rows, present, want, ok = rrc.blob(kind, log2_n, log2_l, bitrev, rng)
                blobs.append((rows, present, want, ok))
            labels.append(kind)
        return pack(blobs, log2_n, labels)
    return rc._cached(("forgery-mixed", log2_n, log2_l, bitrev), build)


def structured_instance(log2_n, log2_l, bitrev):
    """field values with structure: f = 0 (ok = 1 and a zero row: not the blob with too few cells beside it), f constant, every coefficient
    r - 1, f = X^(N-1), zero cells with exactly k present, the values of STRUCTURED as coefficients; under several patterns each"""
    def build():
        rng = random.Random(0x57 + 8 * log2_n + log2_l + bitrev)
        n_co, l, k, _, big_m, _ = rm.sizes(log2_n, log2_l)
        polys = [("zero", [0] * n_co), ("constant", [rng.randrange(1, R)] + [0] * (n_co - 1)), ("all r-1", [R - 1] * n_co), ("top", [0] * (n_co - 1) + [1]),
                 ("structured", [STRUCTURED[i % len(STRUCTURED)] for i in range(n_co)]), ("structured-reversed", [STRUCTURED[-1 - i % len(STRUCTURED)] for i in range(n_co)])]
        blobs, labels = [], []
        for name, f in polys:
            cells = rm.cells_of(f, log2_n, log2_l, bitrev)
            for kind in ("none", "one", "random-half", "first-half", "odd"):
                blobs.append((cells, rm.pattern(kind, big_m, rng), f, 1))
                labels.append("%s %s" % (name, kind))
            blobs.append((cells, keep_cells(big_m, k - 1, rng), [0] * n_co, 0))
            labels.append("%s few" % name)
        zero = [[0] * l for _ in range(big_m)]
        for _ in range(2):
            blobs.append((zero, keep_cells(big_m, k, rng), [0] * n_co, 1))
            labels.append("zero cells, exactly k present")
        return pack(blobs, log2_n, labels)
    return rc._cached(("forgery-structured", log2_n, log2_l, bitrev), build)


# ------------------------------------------------------------------------------------------------------------------- the kernels on host threads
def ints(rows):
    return pm.from_bytes(np.ascontiguousarray(rows, dtype=np.uint64).tobytes())


def kernel_host_input(inst, log2_n, log2_l, bitrev):
    """an instance as the input file of tests/recover_kernel_host.cpp: present | the inverse size-l transforms of the present cells (missing
    ones as they are) | Z on the roots | Z on the coset, where Z is zero for a blob with too few cells - what the driver's borrowed
    transforms hand to the three kernels, from the model.  -> (bytes, the ok flags k_rec_vanish must leave)"""
    _, l, k, _, big_m, mu = rm.sizes(log2_n, log2_l)
    n = inst["ok"].size
    pres = inst["present"].reshape(n, big_m)
    vals = inst["values"].reshape(n, big_m, l, 4)
    mp = [pm.bit_reverse(m, mu) if bitrev else m for m in range(big_m)]
    coef, zr, zs, enough, tables = [], [], [], [], {}
    for j in range(n):
        key = (pres[j] != 0).tobytes()
        if key not in tables:
            ok = int((pres[j] != 0).sum()) >= k
            z = rm.vanishing([mp[m] for m in range(big_m) if not pres[j, m]], mu) if ok else [0] * big_m
            tables[key] = (pm.to_bytes(pm.ntt(z, mu)), pm.to_bytes(pm.ntt(z, mu, coset=True)), int(ok))
        zr.append(tables[key][0])
        zs.append(tables[key][1])
        enough.append(tables[key][2])
        for m in range(big_m):
            coef.append(pm.to_bytes(pm.ntt(ints(vals[j, m]), log2_l, inverse=True, bitrev=bitrev)) if pres[j, m] else vals[j, m].tobytes())
    return pres.tobytes() + b"".join(coef) + b"".join(zr) + b"".join(zs), np.array(enough, dtype=np.int32)


def kernel_host_output(raw, n, log2_n, log2_l):
    """the output file -> (ok after k_rec_vanish, coefficients (n N, 4), ok after k_rec_column)"""
    n_co, _, _, _, big_m, _ = rm.sizes(log2_n, log2_l)
    assert len(raw) == 2 * 32 * n * big_m + 4 * n + 32 * n * n_co + 4 * n
    at = 32 * n * big_m
    ok_vanish = np.frombuffer(raw[at:at + 4 * n], dtype=np.int32)
    at = 2 * at + 4 * n
    return ok_vanish, np.frombuffer(raw[at:at + 32 * n * n_co], dtype=np.uint64).reshape(-1, 4), np.frombuffer(raw[-4 * n:], dtype=np.int32)
