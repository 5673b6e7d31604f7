"""Inputs for the calls that cut themselves into slices (helper of test_slices_cpu.py and test_gpu_slices.py; not a test module): the G1
NTT and FK20 (csrc/zkp_fk20.hip) and the KZG opening (csrc/zkp_poly.hip) walk `for (at = 0; at < n; at += slice)` and add an offset made
from `at` to every operand.  A call large enough to cross a slice boundary is too large to compute item by item on the CPU, so it is
ASSEMBLED: a small pool of B distinct items (B prime, so no slice length is a multiple of it) with their expected outputs - Python
integers of poly_model / fk20_model and one oracle multiplication of the generator per point (replay_cases.expect_points), nothing from
the library under test - and a seeded pseudo-random index sequence idx over the pool; item j of the call is pool item idx[j], inputs and
expected outputs alike, by numpy indexing.  The last `tail` items of a call, its short last slice, are pool items used nowhere else in it.

The slice conditions.  A sliced entry point is tested by its GPU test only if all of these hold, and test_slices_cpu.py checks them
without a GPU for every Call made here; the next sliced entry point gets a pool here and the same checks there:
  1. slice sizes: the slice length the test assumes is what the planning header computes for the exact shape (a few lines of C++ that
     print it), and it equals the header's documented formula; the shape gives the intended number of slices with a short, non-empty
     last one.  Whoever changes a slice constant sees the CPU test fail instead of a GPU test that no longer crosses a boundary.
  2. no shift invariance: for every slice start at > 0 and w = min(64, slice length) items (the slice's own length if it is shorter), the
     rows [at, at + w) of EVERY input and EVERY expected output array differ from the rows [0, w) and from those of every other start.
  3. mutations: the expected arrays read as a wrong build would fill them - slice s taken from offset 0, slice s taken from the offset of
     slice s - 1 - differ from the true expected bytes in EVERY output array of the call (points and flags; y, proofs and flags).
  4. the pool is consistent on integers by a second route (the inverse transform gives the vector back, the circulant pipeline equals
     the quotient formula, y in the domain is the evaluation of that slot), and the assembled rows decode to the pool's values.
Condition 3 on the opening's flags needs identity proofs, which dense random polynomials never give: its pool holds two constant
polynomials and the zero polynomial next to the dense ones, one of the constants in the tail.  The seeds below are ones for which the
conditions hold (three flag bytes of a tail can equal the first three of a call by chance): they are properties of the inputs alone, and
test_slices_cpu.py is their judge - change a seed or a shape, run it.

Hash-to-G2 and the BLS verifier (csrc/zkp_bls.hip; the last section) follow the same pattern on messages, pairs of field elements and
signatures, with the model of tests/h2c_model.py behind the expected bytes.  Two departures, both stated where they occur: the flags of
hash_to_g2 are zero everywhere (no message hashes to the identity), so condition 3 holds for its points only; and the verifier returns
one verdict, so conditions 2 and 3 are checked on the array its slices write, the hashed points, and the GPU test moves a forgery across
the boundary instead.

Hash-to-G1 and the min-sig verifiers (csrc/zkp_bls_minsig.hip) have the same five kinds of call with tests/h2g1_model.py behind them, and
the grouped and the committee verifier (csrc/zkp_bls_grouped.hip, csrc/zkp_bls_agg.hip), which drive sliced callees on m messages or n
aggregate keys, a call each above 2^17: the last two sections."""
import random

import numpy as np

import fk20_model as fm
import fk20_replay_cases as frc
import poly_model as pm
import poly_replay_cases as prc
import replay_cases as rc
from replay_cases import fr_rows

R = pm.R
TAU = prc.TAU
SEED = 0x511CE5
WINDOW = 64

# the shapes: the smallest that the ABI's slice sizes allow (csrc/zkp_fk20_plan.hpp, csrc/zkp_poly_plan.hpp)
NTT_LOG2 = 3                                     # the first size with two twiddled stages
NTT_SLICE = (1 << 18) >> NTT_LOG2                # floor(2^18 / N) vectors
NTT_N_VEC = 2 * NTT_SLICE + 5                    # three slices, the last of 5 vectors: 20 butterflies, a partial wavefront
FK20_LOG2 = 2
FK20_SLICE = (1 << 17) >> FK20_LOG2              # floor(2^17 / N) polynomials: a slice holds 2 N records each
FK20_N = FK20_SLICE + 3
OPEN_LOG2 = 10
OPEN_SLICE = (1 << 22) >> OPEN_LOG2              # floor(2^22 / N) polynomials
OPEN_N = OPEN_SLICE + 3


class Call:
    """one assembled call: n items in slices of `slice` items; inputs / outputs: name -> (array, rows of one item); idx: the pool item
    of every item (the opening: of its polynomial); pool: whatever the builder keeps of the integers"""

    def __init__(self, n, slice, idx, inputs, outputs, pool):
        self.n, self.slice, self.idx, self.inputs, self.outputs, self.pool = n, slice, idx, inputs, outputs, pool
        self.starts = list(range(0, n, slice))
        self.tail = n - self.starts[-1]

    def arg(self, name):
        return self.inputs[name][0]

    def want(self, name):
        return self.outputs[name][0]


def rows(arr, per, at, cnt):
    """the rows of items [at, at + cnt)"""
    return arr[at * per:(at + cnt) * per]


def window(call, at):
    return min(WINDOW, call.slice, call.n - at)


def reading(call, name, how):
    """the expected array `name` as a build with a wrong offset in slice s > 0 would leave it: 'zero' - every later slice computed from,
    or written over, offset 0; 'previous' - from the offset of the slice before it"""
    arr, per = call.outputs[name]
    out = arr.copy()
    for s, at in enumerate(call.starts):
        if s == 0:
            continue
        cnt = min(call.slice, call.n - at)
        src = 0 if how == "zero" else call.starts[s - 1]
        out[at * per:(at + cnt) * per] = rows(arr, per, src, cnt)
    return out


def first_difference(got, want, per, call):
    """(item, slice, pool item) of the first item whose rows differ, or None: what a failing byte comparison reports"""
    got, want = np.ascontiguousarray(got).reshape(call.n, -1), np.ascontiguousarray(want).reshape(call.n, -1)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, per)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if not bad.size:
        return None
    j = int(bad[0])
    return dict(item=j, slice=j // call.slice, offset_in_slice=j % call.slice, pool_item=int(call.idx[j]), items_wrong=int(bad.size))


def draw(seed, n, tail_ids, n_pool):
    """idx: the tail ids at the end in their order, everything before them drawn from the other pool items"""
    body = np.array([j for j in range(n_pool) if j not in tail_ids], dtype=np.int64)
    idx = body[np.random.RandomState(seed).randint(0, len(body), size=n)]
    idx[n - len(tail_ids):] = tail_ids
    return idx


def take(arr, n_pool, idx):
    """pool array (n_pool * per, ...) -> call array (len(idx) * per, ...)"""
    a = arr.reshape((n_pool, -1))
    return a[idx].reshape((-1,) + arr.shape[1:])


def _distinct(items):
    assert len({tuple(x) for x in items}) == len(items)


# ------------------------------------------------------------------------------------------------------------------- the G1 NTT
NTT_B = 13
NTT_TAIL = (8, 9, 10, 11, 12)


def ntt_kinds(finite=False):
    """VECTOR_KINDS cycled; a second all-identity vector would equal the first, so later ones are "holes".  finite: no identity entry in
    any INPUT (the call with inf = NULL)"""
    if finite:
        return [("random", "constant", "spike")[j % 3] for j in range(NTT_B)]
    kinds = [frc.VECTOR_KINDS[j % 5] for j in range(NTT_B)]
    return [("holes" if k == "identity" and j >= 5 else k) for j, k in enumerate(kinds)]


def ntt_pool(flags, finite=False):
    def build():
        rng = random.Random(SEED * 3 + flags + (8 if finite else 0))
        kinds = ntt_kinds(finite)
        vecs = [frc.make_vector(k, NTT_LOG2, flags, rng) for k in kinds]
        _distinct(vecs)
        outs = [pm.ntt_flags(v, NTT_LOG2, flags) for v in vecs]
        pts, inf, out, out_inf = frc.ntt_io(vecs, NTT_LOG2, flags)
        return dict(kinds=kinds, vecs=vecs, outs=outs, points=pts, inf=inf, out=out, out_inf=out_inf)
    return rc._cached(("slice-ntt-pool", flags, finite), build)


def ntt_call(flags, finite=False):
    p = ntt_pool(flags, finite)
    idx = draw(SEED + 11 * flags + finite, NTT_N_VEC, NTT_TAIL, NTT_B)
    per = 1 << NTT_LOG2
    inputs = dict(points=(take(p["points"], NTT_B, idx), per), inf=(take(p["inf"], NTT_B, idx), per))
    outputs = dict(out=(take(p["out"], NTT_B, idx), per), out_inf=(take(p["out_inf"], NTT_B, idx), per))
    return Call(NTT_N_VEC, NTT_SLICE, idx, inputs, outputs, p)


# ------------------------------------------------------------------------------------------------------------------- FK20
FK20_B = 11
FK20_TAIL = (7, 9, 10)                           # constant, ends, random: identity proofs on both sides of the boundary


def fk20_kinds():
    """POLY_KINDS cycled; a second zero polynomial would equal the first, so it is a constant (every proof the identity as well)"""
    kinds = [frc.POLY_KINDS[j % 5] for j in range(FK20_B)]
    return [("constant" if k == "zero" and j >= 5 else k) for j, k in enumerate(kinds)]


def fk20_pool(bitrev):
    def build():
        rng = random.Random(SEED * 5 + bitrev)
        kinds = fk20_kinds()
        polys = [frc.make_poly(k, 1 << FK20_LOG2, rng) for k in kinds]
        _distinct(polys)
        exps = [fm.quotient_proofs(f, TAU, FK20_LOG2, bitrev) for f in polys]
        proof, inf = rc.expect_points(1, [e for x in exps for e in x])
        return dict(kinds=kinds, polys=polys, exps=exps, coeffs=fr_rows([v for f in polys for v in f]), proof=proof, inf=inf)
    return rc._cached(("slice-fk20-pool", bitrev), build)


def fk20_call(bitrev):
    p = fk20_pool(bitrev)
    idx = draw(SEED + 101 + bitrev, FK20_N, FK20_TAIL, FK20_B)
    per = 1 << FK20_LOG2
    inputs = dict(coeffs=(take(p["coeffs"], FK20_B, idx), per))
    outputs = dict(proof=(take(p["proof"], FK20_B, idx), per), inf=(take(p["inf"], FK20_B, idx), per))
    return Call(FK20_N, FK20_SLICE, idx, inputs, outputs, p)


# ------------------------------------------------------------------------------------------------------------------- the opening
OPEN_B, OPEN_C = 13, 12
OPEN_POLY_KINDS = ["random"] * OPEN_B
OPEN_POLY_KINDS[3], OPEN_POLY_KINDS[6], OPEN_POLY_KINDS[11] = "constant", "zero", "constant"
OPEN_TAIL = (10, 11, 12)                         # the polynomials of the tail: dense, constant, dense ..
OPEN_Z_KINDS = prc.Z_KINDS + ("outside",) * (OPEN_C - len(prc.Z_KINDS))
OPEN_TAIL_Z = (4, 0, 2)                          # .. at slotlast, outside, slot0
IN_DOMAIN_Z = tuple(c for c, k in enumerate(OPEN_Z_KINDS) if k.startswith("slot"))


class SlotSetup:
    """what poly_replay_cases.Setup holds, without an engine: the Lagrange points come from the oracle"""

    def __init__(self, log2_n, bitrev):
        self.log2_n, self.bitrev, self.n = log2_n, bitrev, 1 << log2_n
        order = [pm.bit_reverse(i, log2_n) if bitrev else i for i in range(self.n)]
        dom = pm.domain(log2_n)
        lag = fm.lagrange_at(TAU, log2_n)
        natural = rc._cached(("slice-lagrange", log2_n), lambda: rc.expect_points(1, lag)[0])
        self.order = order
        self.slot_domain = [dom[i] for i in order]
        self.lagrange_tau = [lag[i] for i in order]
        self.lagrange_g1 = np.ascontiguousarray(natural[order])


def open_pool(bitrev):
    def build():
        rng = random.Random(SEED * 7)            # the same polynomials for both orders; the in-domain points differ
        st = SlotSetup(OPEN_LOG2, bitrev)
        polys = [prc.make_poly(k, st.n, rng) for k in OPEN_POLY_KINDS]
        _distinct(polys)
        zs = [prc.make_z(k, st, rng) for k in OPEN_Z_KINDS]
        assert len(set(zs)) == OPEN_C
        natural = rc._cached(("slice-open-evals",), lambda: [pm.ntt(f, OPEN_LOG2) for f in polys])
        evals = [[e[i] for i in st.order] for e in natural]
        f_tau = [prc.horner(f, TAU) for f in polys]
        y = [[prc.horner(f, z) for z in zs] for f in polys]
        q = [[(f_tau[p] - y[p][c]) * pow(TAU - zs[c], -1, R) % R for c in range(OPEN_C)] for p in range(OPEN_B)]
        proof, inf = rc.expect_points(1, [e for x in q for e in x])
        commit, cinf = rc.expect_points(1, f_tau)
        return dict(setup=st, polys=polys, zs=zs, evals_int=evals, y_int=y, q=q, f_tau=f_tau, evals=fr_rows([v for e in evals for v in e]), z=fr_rows(zs),
                    y=fr_rows([v for x in y for v in x]), proof=proof, inf=inf, commit=commit, cinf=cinf)
    return rc._cached(("slice-open-pool", bitrev), build)


def open_call(bitrev):
    """Call.idx is the polynomial of every opening, Call.iz its point; the evaluations are 128 MiB, so nothing here is cached"""
    p = open_pool(bitrev)
    idx = draw(SEED + 211 + bitrev, OPEN_N, OPEN_TAIL, OPEN_B)
    iz = np.random.RandomState(SEED + 301 + bitrev).randint(0, OPEN_C, size=OPEN_N)
    iz[OPEN_N - len(OPEN_TAIL_Z):] = OPEN_TAIL_Z
    pair = idx * OPEN_C + iz
    inputs = dict(evals=(take(p["evals"], OPEN_B, idx), 1 << OPEN_LOG2), z=(p["z"][iz], 1))
    outputs = dict(y=(p["y"][pair], 1), proof=(p["proof"][pair], 1), inf=(p["inf"][pair], 1))
    call = Call(OPEN_N, OPEN_SLICE, idx, inputs, outputs, p)
    call.iz = iz
    return call


# ------------------------------------------------------------------------------------------------------------------- hash-to-G2 and the BLS verifier
# csrc/zkp_bls.hip walks the messages (or the pairs of field elements) in slices of bls::SLICE; the u values and the projective points of a
# slice overwrite those of the slice before it, and the stride of the point workspace is twice the slice length of the CALL.  The last slice
# of a hash call is longer than any pool (61 items, a partial wavefront of k_h2c_clear), so it is drawn from four pool items that occur
# nowhere before it; the tails of the map and of the verifier are distinct items like the ones above.
BLS_SLICE = 1 << 17
BLS_B = 13
HASH_N = BLS_SLICE + 61
HASH_LENGTHS = (0, 1, 55, 56, 64, 119, 120, 8, 9, 72, 73, 17, 37)   # the empty message; 8 | 9 and 72 | 73 are where b_0 (43-byte tag) gains a block
HASH_TAIL = (3, 8, 10, 12)                                           # 56, 9, 73 and 37 bytes
HASH_BASE = 5                                                        # offsets[0]: the messages do not start at the buffer's first byte
MAP_N = 2 * BLS_SLICE + 5
MAP_TAIL = (8, 9, 10, 11, 12)
MAP_INF = 10                                                         # the pair (a, -a): the identity, in the tail
MAP_INF_BODY = 3                                                     # another such pair, so that the flags of the full slices differ as well
VERIFY_N = BLS_SLICE + 6
VERIFY_TAIL = (7, 8, 9, 10, 11, 12)
VERIFY_BASE = 3


def draw_spread(seed, n, tail, tail_ids, n_pool):
    """idx: the last `tail` items drawn from tail_ids (each at least once), everything before them from the other pool items"""
    body = np.array([j for j in range(n_pool) if j not in tail_ids], dtype=np.int64)
    idx = body[np.random.RandomState(seed).randint(0, len(body), size=n)]
    ids = np.array(tail_ids, dtype=np.int64)
    last = ids[np.random.RandomState(seed + 1).randint(0, len(ids), size=tail)]
    last[:len(ids)] = ids
    idx[n - tail:] = last
    return idx


def pack_from_pool(msgs, idx, base):
    """the messages idx of the pool as one buffer behind `base` filler bytes -> (buffer, offsets (n + 1,), rows): rows (n, width + 1) are
    the messages zero-padded to one width with the length in the last column, the fixed-width form the slice conditions are checked on"""
    width = max(len(x) for x in msgs)
    assert width < 256
    mat = np.zeros((len(msgs), width + 1), dtype=np.uint8)
    for j, x in enumerate(msgs):
        mat[j, :len(x)] = np.frombuffer(x, dtype=np.uint8)
        mat[j, width] = len(x)
    rows = mat[idx]
    lens = rows[:, width].astype(np.uint64)
    off = np.full(len(idx) + 1, base, dtype=np.uint64)
    off[1:] += np.cumsum(lens, dtype=np.uint64)
    keep = np.arange(width, dtype=np.uint64)[None, :] < lens[:, None]
    buf = np.concatenate([np.full(base, 0xA5, dtype=np.uint8), rows[:, :width][keep]])
    return buf, off, rows


def hash_pool():
    def build():
        import bls_replay_cases as brc
        rng = random.Random(SEED * 11)
        msgs = [bytes(rng.randrange(256) for _ in range(k)) for k in HASH_LENGTHS]
        _distinct(msgs)
        pts = [brc.hashed(x, brc.DST) for x in msgs]
        points, inf = brc.point_rows(pts)
        return dict(msgs=msgs, pts=pts, u=brc.field_rows(msgs, brc.DST), points=points, inf=inf)
    return rc._cached(("slice-hash-pool",), build)


def hash_call(points):
    """hash_to_g2 (points and flags) or hash_to_field_g2 (u) on SLICE + 61 messages; Call.msgs / Call.offsets are the arguments"""
    p = hash_pool()
    idx = draw_spread(SEED + 401 + points, HASH_N, HASH_N - BLS_SLICE, HASH_TAIL, BLS_B)
    buf, off, rows = pack_from_pool(p["msgs"], idx, HASH_BASE)
    outputs = dict(points=(p["points"][idx], 1), inf=(p["inf"][idx], 1)) if points else dict(u=(p["u"][idx], 1))
    call = Call(HASH_N, BLS_SLICE, idx, dict(msg=(rows, 1)), outputs, p)
    call.msgs, call.offsets = buf, off
    call.constant = {"inf"} if points else set()     # no message hashes to the identity: the flags are zero in every slice
    return call


def map_pool():
    def build():
        import bls12_381_model as m
        import bls_replay_cases as brc
        import h2c_model as h
        g = m.SplitMix64(SEED * 13)
        us = [((g.below(h.P), g.below(h.P)), (g.below(h.P), g.below(h.P))) for _ in range(BLS_B)]
        for j in (MAP_INF, MAP_INF_BODY):
            us[j] = (us[j][0], m.f2_neg(us[j][0]))
        _distinct(us)
        pts = [h.map_from_fields(a, b) for a, b in us]
        points, inf = brc.point_rows(pts)
        return dict(us=us, pts=pts, u=brc.u64([h.f2_words(a) + h.f2_words(b) for a, b in us]).reshape(-1, 24), points=points, inf=inf)
    return rc._cached(("slice-map-pool",), build)


def map_call():
    p = map_pool()
    idx = draw(SEED + 501, MAP_N, MAP_TAIL, BLS_B)
    call = Call(MAP_N, BLS_SLICE, idx, dict(u=(p["u"][idx], 1)), dict(points=(p["points"][idx], 1), inf=(p["inf"][idx], 1)), p)
    call.constant = set()
    return call


def verify_pool():
    def build():
        import bls_replay_cases as brc
        import h2c_model as h
        pool = brc.signed_pool()[:BLS_B]         # all 16 would make the slice a multiple of the pool size
        msgs = [x[2] for x in pool]
        _distinct(msgs)
        hq, hinf = brc.point_rows([brc.hashed(x, brc.DST) for x in msgs])
        assert not hinf.any()
        return dict(pool=pool, msgs=msgs, pk=brc.u64([h.g1_words(x[1])[0] for x in pool]).reshape(-1, 12),
                    sig=brc.u64([h.g2_words(x[3])[0] for x in pool]).reshape(-1, 24), hq=hq)
    return rc._cached(("slice-verify-pool",), build)


def verify_call():
    """bls_verify on SLICE + 6 valid signatures.  The call's one output is a verdict; what the slices write is the workspace array of hashed
    points, so that is the array the conditions are checked on.  Call.forged: the items whose message a test changes, one at a time"""
    p = verify_pool()
    idx = draw(SEED + 601, VERIFY_N, VERIFY_TAIL, BLS_B)
    buf, off, rows = pack_from_pool(p["msgs"], idx, VERIFY_BASE)
    rand = np.random.RandomState(SEED + 602).randint(1, 1 << 62, size=(VERIFY_N, 2)).astype(np.uint64)
    inputs = dict(pk=(p["pk"][idx], 1), sig=(p["sig"][idx], 1), msg=(rows, 1), rand=(rand, 1))
    call = Call(VERIFY_N, BLS_SLICE, idx, inputs, dict(hq=(p["hq"][idx], 1)), p)
    call.msgs, call.offsets, call.constant = buf, off, set()
    call.forged = (BLS_SLICE - 1, BLS_SLICE, VERIFY_N - 1)
    return call


def forged_messages(call, j):
    """the message buffer with the first byte of message j changed (message j is not empty: test_slices_cpu.py)"""
    buf = call.msgs.copy()
    buf[int(call.offsets[j])] ^= 1
    return buf


def message_list(call, msgs=None):
    """the call's messages as a list of bytes, for the entry points that take one"""
    buf = (call.msgs if msgs is None else msgs).tobytes()
    off = call.offsets.tolist()
    return [buf[a:b] for a, b in zip(off[:-1], off[1:])]


# ------------------------------------------------------------------------------------------------------------------- hash-to-G1 and the min-sig verifiers
# csrc/zkp_bls_minsig.hip walks its messages, pairs of field elements and points in slices of minsig::SLICE = bls::SLICE, like the section
# above, with tests/h2g1_model.py behind the expected bytes.  The shapes, the message lengths and the tails are those of the hash-to-G2
# calls; the pools are others (other seeds, the other tag).  The cofactor call takes its points from h2g1_adversarial.point_cases(): points
# of small order and two flagged identities make its output flags differ on both sides of every boundary.  The verifiers are judged on
# the hashed G1 points, the array their slices write (the same-key verifier writes them into every second row of its columns).
CLEAR_NAMES = ("order3_plus", "order3_minus", "identity", "order11", "g1_random", "g1_generator", "g1_negated", "order3_plus_g1",
               "order11_plus_g1", "order33_plus_g1", "flagged_generator", "outside0", "outside1")
CLEAR_FLAGGED_BODY, CLEAR_FLAGGED_TAIL = 2, 10                        # (0, 1) with its flag; the generator's words with the flag, which decides


def minsig_field_pool():
    def build():
        import minsig_replay_cases as mrc
        rng = random.Random(SEED * 17)
        msgs = [bytes(rng.randrange(256) for _ in range(k)) for k in HASH_LENGTHS]
        _distinct(msgs)
        return dict(msgs=msgs, u=mrc.field_rows(msgs, mrc.DST))
    return rc._cached(("slice-minsig-field-pool",), build)


def minsig_field_call():
    """hash_to_field_g1 on SLICE + 61 messages; Call.msgs / Call.offsets are the arguments"""
    p = minsig_field_pool()
    idx = draw_spread(SEED + 701, HASH_N, HASH_N - BLS_SLICE, HASH_TAIL, BLS_B)
    buf, off, rows = pack_from_pool(p["msgs"], idx, HASH_BASE)
    call = Call(HASH_N, BLS_SLICE, idx, dict(msg=(rows, 1)), dict(u=(p["u"][idx], 1)), p)
    call.msgs, call.offsets, call.constant = buf, off, set()
    return call


def minsig_map_pool():
    def build():
        import h2g1_model as g
        import minsig_replay_cases as mrc
        rng = random.Random(SEED * 19)
        us = [(rng.randrange(1, g.P), rng.randrange(1, g.P)) for _ in range(BLS_B)]
        for j in (MAP_INF, MAP_INF_BODY):
            us[j] = (us[j][0], g.P - us[j][0])
        _distinct(us)
        pts = [g.map_from_fields(a, b) for a, b in us]
        points, inf = mrc.point_rows(pts)
        return dict(us=us, pts=pts, u=mrc.u64([g.fp_words(a) + g.fp_words(b) for a, b in us]).reshape(-1, 12), points=points, inf=inf)
    return rc._cached(("slice-minsig-map-pool",), build)


def minsig_map_call():
    p = minsig_map_pool()
    idx = draw(SEED + 711, MAP_N, MAP_TAIL, BLS_B)
    call = Call(MAP_N, BLS_SLICE, idx, dict(u=(p["u"][idx], 1)), dict(points=(p["points"][idx], 1), inf=(p["inf"][idx], 1)), p)
    call.constant = set()
    return call


def minsig_clear_pool():
    def build():
        import h2g1_adversarial as ha
        import h2g1_model as g
        import minsig_replay_cases as mrc
        by = dict(ha.point_cases())
        by["flagged_generator"] = None
        pts = [by[k] for k in CLEAR_NAMES]
        rows, flags = mrc.point_rows(pts)
        rows[CLEAR_FLAGGED_TAIL] = mrc.u64(g.g1_words(g.m.G1_GEN)[0])
        assert flags.tolist() == [int(j in (CLEAR_FLAGGED_BODY, CLEAR_FLAGGED_TAIL)) for j in range(BLS_B)]
        _distinct([r.tolist() + [f] for r, f in zip(rows, flags)])
        outs = [g.clear_cofactor(q) for q in pts]
        points, inf = mrc.point_rows(outs)
        return dict(names=CLEAR_NAMES, pts=pts, outs=outs, pts_rows=rows, pts_inf=flags, points=points, inf=inf)
    return rc._cached(("slice-minsig-clear-pool",), build)


def minsig_clear_call():
    p = minsig_clear_pool()
    idx = draw(SEED + 723, MAP_N, MAP_TAIL, BLS_B)
    call = Call(MAP_N, BLS_SLICE, idx, dict(pts=(p["pts_rows"][idx], 1), inf=(p["pts_inf"][idx], 1)), dict(points=(p["points"][idx], 1), inf=(p["inf"][idx], 1)), p)
    call.constant = set()
    return call


def minsig_verify_pool(same_key):
    """BLS_B messages signed by g.sign: by BLS_B keys, or all by one"""
    def build():
        import h2c_model as h
        import h2g1_model as g
        import minsig_replay_cases as mrc
        rng = random.Random(SEED * 29 + same_key)
        one = rng.randrange(1, g.R_ORDER)
        pool = []
        for _ in range(BLS_B):
            sk = one if same_key else rng.randrange(1, g.R_ORDER)
            msg = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 48)))
            pool.append((sk, g.sk_to_pk(sk), msg, g.sign(sk, msg, mrc.DST)))
        msgs = [x[2] for x in pool]
        _distinct(msgs)
        hp, hinf = mrc.point_rows([mrc.hashed(x, mrc.DST) for x in msgs])
        assert not hinf.any()
        return dict(pool=pool, msgs=msgs, pk=mrc.u64([h.g2_words(x[1])[0] for x in pool]).reshape(-1, 24),
                    sig=mrc.u64([g.g1_words(x[3])[0] for x in pool]).reshape(-1, 12), hp=hp)
    return rc._cached(("slice-minsig-verify-pool", same_key), build)


def minsig_verify_call(same_key):
    """bls_minsig_verify or bls_minsig_verify_samekey on SLICE + 6 valid signatures, judged on the hashed points as verify_call is.  For the
    same-key call Call.pk1 is the one key; its input pk repeats it and is constant"""
    p = minsig_verify_pool(same_key)
    idx = draw(SEED + 731 + same_key, VERIFY_N, VERIFY_TAIL, BLS_B)
    buf, off, rows = pack_from_pool(p["msgs"], idx, VERIFY_BASE)
    rand = np.random.RandomState(SEED + 741 + same_key).randint(1, 1 << 62, size=(VERIFY_N, 2)).astype(np.uint64)
    inputs = dict(sig=(p["sig"][idx], 1), msg=(rows, 1), rand=(rand, 1))
    if not same_key:
        inputs["pk"] = (p["pk"][idx], 1)
    call = Call(VERIFY_N, BLS_SLICE, idx, inputs, dict(hp=(p["hp"][idx], 1)), p)
    call.msgs, call.offsets, call.constant = buf, off, set()
    call.pk1 = np.ascontiguousarray(p["pk"][:1])
    call.forged = (BLS_SLICE - 1, BLS_SLICE, VERIFY_N - 1)
    call.shifted = BLS_SLICE + 2                                     # the signature a test moves out of G1: its status byte lies behind the boundary
    call.flagged_pk = BLS_SLICE + 1
    return call


def shifted_signature(call, j):
    """the signatures with number j moved by (0, 2), a point of order 3: on the curve, outside G1, and the pairing equation still holds"""
    import h2g1_model as g
    import minsig_replay_cases as mrc
    sig = call.arg("sig").copy()
    moved = g.e_add(call.pool["pool"][call.idx[j]][3], (0, 2))
    sig[j] = mrc.u64(g.g1_words(moved)[0])
    return sig, moved


# ------------------------------------------------------------------------------------------------------------------- the grouped and the committee verifiers
# csrc/zkp_bls_grouped.hip and csrc/zkp_bls_agg.hip do not slice themselves; they drive sliced callees on workspace arrays: the hash on m
# messages, bls_verify on the n aggregate keys, the Miller product over m pairs.  Their calls are judged on what those callees write.
GROUPED_M = BLS_SLICE + 6
GROUPED_SIZES = {5: 0, 6: 2, BLS_SLICE - 2: 0, BLS_SLICE: 3}          # every other group holds one signature: n = m + 1
COM_N = BLS_SLICE + 6
COM_TABLE = 36
COM_SIZES = (1, 2, 3, 4, 5, 7, 33, 2, 1, 3, 5, 4, 7)                  # 33: a run border (32 records) inside a committee, in the body
COM_WIDTH = max(COM_SIZES)


def grouped_call():
    """bls_verify_grouped on m = SLICE + 6 messages: group g holds the key and the signature of pool item idx[g] of verify_pool(), once,
    but for the groups of GROUPED_SIZES, which hold it 0, 2, 0 and 3 times.  Call.n is m, the count its sliced callee walks; Call.pk,
    Call.sig, Call.rand and Call.grp_off are the arguments per signature, Call.member the group of every signature"""
    p = verify_pool()
    m = GROUPED_M
    idx = draw(SEED + 801, m, VERIFY_TAIL, BLS_B)
    buf, off, rows = pack_from_pool(p["msgs"], idx, VERIFY_BASE)
    sizes = np.ones(m, dtype=np.int64)
    for g, k in GROUPED_SIZES.items():
        sizes[g] = k
    grp_off = np.zeros(m + 1, dtype=np.uint64)
    grp_off[1:] = np.cumsum(sizes).astype(np.uint64)
    member = np.repeat(np.arange(m, dtype=np.int64), sizes)
    rand = np.random.RandomState(SEED + 802).randint(1, 1 << 62, size=(member.size, 2)).astype(np.uint64)
    call = Call(m, BLS_SLICE, idx, dict(msg=(rows, 1), pk=(p["pk"][idx], 1), sig=(p["sig"][idx], 1)), dict(hq=(p["hq"][idx], 1)), p)
    call.msgs, call.offsets, call.constant = buf, off, set()
    call.sizes, call.grp_off, call.member, call.rand = sizes, grp_off, member, rand
    call.pk, call.sig = np.ascontiguousarray(p["pk"][idx[member]]), np.ascontiguousarray(p["sig"][idx[member]])
    call.forged = (BLS_SLICE - 1, BLS_SLICE + 1, m - 1)
    call.moved = BLS_SLICE + 1                                       # grp_off[moved] + 1: the signature of this group is filed under the group before it
    return call


def expanded_messages(call, msgs=None):
    """(buffer, offsets) of the grouped call's messages, one per signature: what bls_verify takes"""
    import bls_replay_cases as brc
    lst = message_list(call, msgs)
    return brc.pack([lst[g] for g in call.member.tolist()], VERIFY_BASE)


def committees_pool():
    def build():
        import agg_model as am
        sks, pks = am.key_table(COM_TABLE)
        vp = verify_pool()
        rng = random.Random(SEED * 31)
        entries, sums, sigs = [], [], []
        for j, k in enumerate(COM_SIZES):
            rows = rng.sample(range(COM_TABLE), k)
            neg = [k > 1 and i > 0 and rng.randrange(4) == 0 for i in range(k)]
            sk = sum(-sks[r] if s else sks[r] for r, s in zip(rows, neg)) % am.h.R_ORDER
            assert sk
            entries.append([r | am.SIGN if s else r for r, s in zip(rows, neg)])
            sums.append(sk)
            sigs.append(am.sign(vp["msgs"][j], sk))
        _distinct(entries)
        flat, seg_off = am.committee_entries(entries)
        apk, apk_inf, status = am.sum_rows(pks, flat, seg_off)
        assert not apk_inf.any() and not status.any()
        padded = np.zeros((BLS_B, COM_WIDTH + 1), dtype=np.uint32)
        for j, e in enumerate(entries):
            padded[j, :len(e)], padded[j, COM_WIDTH] = e, len(e)
        return dict(entries=entries, sks=sums, table=am.table_rows(pks), padded=padded, apk=apk, msgs=vp["msgs"], hq=vp["hq"],
                    sig=am.u64([am.h.g2_words(s)[0] for s in sigs]).reshape(-1, 24))
    return rc._cached(("slice-committees-pool",), build)


def committees_call():
    """bls_fast_aggregate_verify on SLICE + 6 committees over a table of 36 keys: committee j of the call is pool committee idx[j] and signs
    pool message idx[j].  Call.entries / Call.seg_off are the committee arguments; the input `com` is their fixed-width form (the entries
    zero-padded, the size in the last column), on which the slice conditions are checked"""
    p = committees_pool()
    idx = draw(SEED + 901, COM_N, VERIFY_TAIL, BLS_B)
    buf, off, rows = pack_from_pool(p["msgs"], idx, VERIFY_BASE)
    com = p["padded"][idx]
    sizes = com[:, COM_WIDTH].astype(np.uint64)
    seg_off = np.zeros(COM_N + 1, dtype=np.uint64)
    seg_off[1:] = np.cumsum(sizes, dtype=np.uint64)
    keep = np.arange(COM_WIDTH, dtype=np.uint64)[None, :] < sizes[:, None]
    rand = np.random.RandomState(SEED + 902).randint(1, 1 << 62, size=(COM_N, 2)).astype(np.uint64)
    call = Call(COM_N, BLS_SLICE, idx, dict(com=(com, 1), msg=(rows, 1), sig=(p["sig"][idx], 1), rand=(rand, 1)),
                dict(apk=(p["apk"][idx], 1), hq=(p["hq"][idx], 1)), p)
    call.msgs, call.offsets, call.constant = buf, off, set()
    call.entries, call.seg_off = np.ascontiguousarray(com[:, :COM_WIDTH][keep]), seg_off
    call.forged = (BLS_SLICE - 1, BLS_SLICE, COM_N - 1)
    return call


def swapped_member(call, j):
    """the entries with the first member of committee j replaced by the lowest table row that the committee does not hold"""
    import agg_model as am
    held = {e & am.ROW for e in call.pool["entries"][call.idx[j]]}
    other = min(r for r in range(COM_TABLE) if r not in held)
    entries = call.entries.copy()
    entries[int(call.seg_off[j])] = other
    return entries, other
