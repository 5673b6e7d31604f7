"""Seeded synthetic inputs: pair i is ([a_i] G1gen, [b_i] G2gen) with scalars from a
SplitMix64 stream.  The scalar multiplications run on the GPU through the engine (zkp_g1_mul_batch /
zkp_g2_mul_batch); nothing here touches oracle/.

The reference's own G1Affine::random / G2Affine::random (src/g1.rs:64-72, src/g2.rs:71-79) return
points that are not on the curve, so they cannot be pairing inputs."""
import numpy as np

SEED = 0x5EEDB15381
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)

G1_GENERATOR = np.array([
    0xfb3af00adb22c6bb, 0x6c55e83ff97a1aef, 0xa14e3a3f171bac58, 0xc3688c4f9774b905, 0x2695638c4fa9ac0f, 0x17f1d3a73197d794,
    0x0caa232946c5e7e1, 0xd03cc744a2888ae4, 0x00db18cb2c04b3ed, 0xfcf5e095d5d00af6, 0xa09e30ed741d8ae4, 0x08b3f481e3aaa0f1,
], dtype=np.uint64)  # reference src/common.rs:92-108
G2_GENERATOR = np.array([
    0xd48056c8c121bdb8, 0x0bac0326a805bbef, 0xb4510b647ae3d177, 0xc6e47ad4fa403b02, 0x260805272dc51051, 0x024aa2b2f08f0a91,
    0xe5ac7d055d042b7e, 0x334cf11213945d57, 0xb5da61bbdc7f5049, 0x596bd0d09920b61a, 0x7dacd3a088274f65, 0x13e02b6052719f60,
    0xe193548608b82801, 0x923ac9cc3baca289, 0x6d429a695160d12c, 0xadfd9baa8cbdd3a7, 0x8cc9cdc6da2e351a, 0x0ce5d527727d6e11,
    0xaaa9075ff05f79be, 0x3f370d275cec1da1, 0x267492ab572e99ab, 0xcb3e287e85a763af, 0x32acd2b02bc28b99, 0x0606c4a02ea734cc,
], dtype=np.uint64)  # reference src/common.rs:110-144
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def splitmix64(seed, count, offset=0):
    """count outputs of SplitMix64(seed), starting at output index `offset` (vectorised)."""
    with np.errstate(over="ignore"):
        idx = np.arange(offset + 1, offset + count + 1, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


_R_LIMBS = np.array([(R_ORDER >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
_ATTEMPTS = 16


def _below_r(w):
    """(n,4) little-endian uint64 values: 0 < value < r, elementwise"""
    lt = np.zeros(w.shape[0], dtype=bool)
    eq = np.ones(w.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (w[:, i] < _R_LIMBS[i])
        eq &= w[:, i] == _R_LIMBS[i]
    return lt & (w != 0).any(axis=1)


def scalars(seed, n, offset=0):
    """(n,4) uint64 scalars, uniform in [1, r) by rejection: scalar i takes the first of its (at most 16)
    255-bit candidates that lies in [1, r); candidate a of scalar i is words 4 (16 i + a) .. + 3 of the SplitMix64 stream,
    so any slice of the sequence can be generated on its own (offset).  A candidate is rejected with probability 0.095."""
    out = np.zeros((n, 4), dtype=np.uint64)
    step = 1 << 15                                    # small blocks: the temporaries stay cache resident
    lane = np.arange(1, 5, dtype=np.uint64)[None, :]
    for lo in range(0, n, step):
        todo = np.arange(lo, min(n, lo + step), dtype=np.int64)
        for a in range(_ATTEMPTS):
            if todo.size == 0:
                break
            with np.errstate(over="ignore"):
                first = (np.uint64(offset) + todo.astype(np.uint64)) * np.uint64(4 * _ATTEMPTS) + np.uint64(4 * a)
                z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (first[:, None] + lane) * np.uint64(0x9E3779B97F4A7C15)
                z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
                z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
                w = z ^ (z >> np.uint64(31))
            w[:, 3] &= np.uint64((1 << 63) - 1)
            good = _below_r(w)
            out[todo[good]] = w[good]
            todo = todo[~good]
        if todo.size:       # probability 4e-17 per scalar
            out[todo] = int_to_scalar(1)
    return out


def scalar_to_int(row):
    return sum(int(x) << (64 * i) for i, x in enumerate(row))


def int_to_scalar(v):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def random_pairs(engine, n, seed=SEED, offset=0, device_tensors=False):
    """n synthetic pairs.  Returns (g1 (n,12), g2 (n,24), a (n,4), b (n,4)); with device_tensors the
    points are torch int64 tensors resident on the engine's GPU."""
    a = scalars(seed, n, 2 * offset)
    b = scalars(seed ^ 0xB5, n, 2 * offset)
    if device_tensors:
        import torch
        dev = torch.device("cuda", engine.device)
        ta = torch.from_numpy(a.view(np.int64)).to(dev)
        tb = torch.from_numpy(b.view(np.int64)).to(dev)
        g1, _ = engine.g1_mul(G1_GENERATOR, ta)
        g2, _ = engine.g2_mul(G2_GENERATOR, tb)
        return g1, g2, a, b
    g1, _ = engine.g1_mul(G1_GENERATOR, a)
    g2, _ = engine.g2_mul(G2_GENERATOR, b)
    return g1, g2, a, b


def below_r(w):
    """(n,4) little-endian uint64 values: value < r (zero included), elementwise - the canonical Fr elements"""
    w = np.asarray(w, dtype=np.uint64).reshape(-1, 4)
    lt = np.zeros(w.shape[0], dtype=bool)
    eq = np.ones(w.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (w[:, i] < _R_LIMBS[i])
        eq &= w[:, i] == _R_LIMBS[i]
    return lt


def _ints(w):
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(w, dtype=np.uint64).reshape(-1, 4)]


def _rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def groth16_instance(seed, n, n_inputs, bad=(), engine=None):
    """A synthetic Groth16 verifying key, n proofs and their public inputs, built from secret exponents (Python integers mod r):
        key    alpha = [a] G1, beta = [b] G2, gamma = [g] G2, delta = [d] G2, IC_i = [k_i] G1 (i <= n_inputs)
        proof  A = [s] G1, B = [t] G2, C = [(s t - a b - g (k_0 + sum_i x_i k_{i+1})) / d] G1
    so that e(A, B) = e(alpha, beta) e(vk_x, gamma) e(C, delta) holds by construction; the proofs listed in `bad` get C + G1 and fail.
    The points come through the engine's g1_mul / g2_mul.  -> (key, proofs, inputs): key = (alpha (12,), beta (24,), gamma (24,),
    delta (24,), ic (n_inputs + 1, 12)), proofs = (A (n,12), B (n,24), C (n,12)), inputs (n, n_inputs, 4) uint64."""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    r, l = R_ORDER, int(n_inputs)
    a, b, g, d = _ints(scalars(seed ^ 0x616, 4))
    k = _ints(scalars(seed ^ 0x1C, l + 1))
    s, t = _ints(scalars(seed ^ 0x0A, n)), _ints(scalars(seed ^ 0x0B, n))
    xw = scalars(seed ^ 0x0C, n * l).reshape(n, l, 4)
    x = _ints(xw)
    dinv = pow(d, r - 2, r)
    bad = set(int(i) for i in bad)
    cexp = []
    for c in range(n):
        vkx = (k[0] + sum(x[c * l + i] * k[i + 1] for i in range(l))) % r
        cexp.append(((s[c] * t[c] - a * b - g * vkx) * dinv + (1 if c in bad else 0)) % r)
    g1s, _ = engine.g1_mul(G1_GENERATOR, _rows([a] + k + s + cexp))
    g2s, _ = engine.g2_mul(G2_GENERATOR, _rows([b, g, d] + t))
    key = (g1s[0].copy(), g2s[0].copy(), g2s[1].copy(), g2s[2].copy(), g1s[1:l + 2].copy())
    proofs = (g1s[l + 2:l + 2 + n].copy(), g2s[3:].copy(), g1s[l + 2 + n:].copy())
    return key, proofs, xw


def groth16_circuit_secrets(seed, log2_n, n_rows, m, n_inputs, n, row_lengths=None, bad=()):
    """The part of groth16_circuit_instance that needs no GPU, on Python integers: a random satisfiable constraint system, n witnesses
    and the trapdoor.  The last n_rows variables are PRODUCT variables: row k has sparse random A and B rows over the variables before
    its product variable p_k = m - n_rows + k (columns drawn with repetition, so a column may repeat inside a row) and the single C
    entry 1 at p_k, which each witness sets to a_k b_k.  row_lengths[k]: the entries of row k in A and in B (default 1 .. 3 at
    random); the first A entries name the constant and the public variables in turn.  Witnesses listed in `bad` get the last product variable off by one.  -> dict: rows_a / rows_b / rows_c (per row, a list
    of (column, value)), z (n lists of m integers), tau alpha beta gamma delta, u_tau v_tau w_tau (the QAP polynomials of every
    variable at tau), log2_n n_rows m n_inputs."""
    import random
    r, big_n, l = R_ORDER, 1 << int(log2_n), int(n_inputs)
    free = m - n_rows
    if n_rows > big_n or free < 1 or l + 1 > m:
        raise ValueError("n_rows <= N, m > n_rows and n_inputs < m are needed")
    rng = random.Random(seed)
    rows_a, rows_b, rows_c = [], [], []
    need = list(range(min(free, l + 1)))[::-1]   # every public variable takes part (the first A entries): a verifying key has no infinite IC_i
    for k in range(n_rows):
        cnt = rng.randrange(1, 4) if row_lengths is None else int(row_lengths[k])
        rows_a.append([(need.pop() if need else rng.randrange(free + k), rng.randrange(1, r)) for _ in range(cnt)])
        rows_b.append([(rng.randrange(free + k), rng.randrange(1, r)) for _ in range(cnt)])
        rows_c.append([(free + k, 1)])
    dot = lambda row, z: sum(v * z[c] for c, v in row) % r
    bad = set(int(j) for j in bad)
    if bad and not n_rows:
        raise ValueError("no constraint to violate")
    zs = []
    for j in range(n):
        z = [1] + [rng.randrange(r) for _ in range(free - 1)] + [0] * n_rows
        for k in range(n_rows):
            z[free + k] = dot(rows_a[k], z) * dot(rows_b[k], z) % r
        if j in bad:
            z[m - 1] = (z[m - 1] + 1) % r
        zs.append(z)
    w = fr_root_of_unity(log2_n)
    while True:
        tau, alpha, beta, gamma, delta = (rng.randrange(1, r) for _ in range(5))
        if pow(tau, big_n, r) != 1:
            break
    scale = (pow(tau, big_n, r) - 1) * pow(big_n, -1, r) % r
    u, v, ww = [0] * m, [0] * m, [0] * m
    wk = 1
    for k in range(n_rows):
        lk = scale * wk % r * pow(tau - wk, -1, r) % r          # l_k(tau)
        for dst, row in ((u, rows_a[k]), (v, rows_b[k]), (ww, rows_c[k])):
            for c, val in row:
                dst[c] = (dst[c] + val * lk) % r
        wk = wk * w % r
    return dict(rows_a=rows_a, rows_b=rows_b, rows_c=rows_c, z=zs, tau=tau, alpha=alpha, beta=beta, gamma=gamma, delta=delta, u_tau=u, v_tau=v, w_tau=ww,
                log2_n=int(log2_n), n_rows=int(n_rows), m=int(m), n_inputs=l)


def csr_arrays(rows):
    """per row a list of (column, value) -> (row_ptr uint32, col uint32, val (nnz, 4) uint64)"""
    row_ptr = np.zeros(len(rows) + 1, dtype=np.uint32)
    row_ptr[1:] = np.cumsum([len(x) for x in rows], dtype=np.uint64)
    col = np.array([c for x in rows for c, _ in x], dtype=np.uint32)
    vals = [v for x in rows for _, v in x]
    return row_ptr, col, _rows(vals) if vals else np.zeros((0, 4), dtype=np.uint64)


def groth16_circuit_instance(seed, log2_n, n_rows, m, n_inputs, n, row_lengths=None, bad=(), engine=None):
    """A synthetic circuit with its Groth16 keys and n witnesses -> (r1cs, pk, vk, witnesses (n, m, 4) uint64, secrets): the constraint
    system, witnesses and trapdoor of groth16_circuit_secrets (returned as `secrets`), the proving key
        a_query_i = [u_i(tau)] g1, b_g1_query_i = [v_i(tau)] g1, b_g2_query_i = [v_i(tau)] g2,
        l_query_i = [(beta u_i + alpha v_i + w_i)(tau) / delta] g1 (i > n_inputs), h_query_i = [tau^i (tau^N - 1) / delta] g1 (i < N - 1)
    with its infinite query entries flagged (a variable absent from A or B), and the verifying key with
    IC_i = [(beta u_i + alpha v_i + w_i)(tau) / gamma] g1.  The points come through the engine's g1_mul / g2_mul."""
    from .pairings import R1CS, Groth16ProvingKey, Groth16VerifyingKey, default_engine
    if engine is None:
        engine = default_engine()
    s = groth16_circuit_secrets(seed, log2_n, n_rows, m, n_inputs, n, row_lengths, bad)
    r, big_n, l = R_ORDER, 1 << int(log2_n), int(n_inputs)
    tau, alpha, beta, gamma, delta = s["tau"], s["alpha"], s["beta"], s["gamma"], s["delta"]
    u, v, w = s["u_tau"], s["v_tau"], s["w_tau"]
    dinv, ginv = pow(delta, -1, r), pow(gamma, -1, r)
    comb = [(beta * u[i] + alpha * v[i] + w[i]) % r for i in range(m)]
    t_tau = (pow(tau, big_n, r) - 1) % r
    lq = [comb[i] * dinv % r for i in range(l + 1, m)]
    hq = [pow(tau, i, r) * t_tau % r * dinv % r for i in range(big_n - 1)]
    ic = [comb[i] * ginv % r for i in range(l + 1)]
    g1e = [alpha, beta, delta] + u + v + lq + hq + ic
    g1s, g1i = engine.g1_mul(G1_GENERATOR, _rows(g1e))
    g2s, g2i = engine.g2_mul(G2_GENERATOR, _rows([beta, gamma, delta] + v))
    at = [3]
    for cnt in (m, m, len(lq), len(hq), len(ic)):
        at.append(at[-1] + cnt)
    cut = lambda i: (g1s[at[i]:at[i + 1]].copy(), np.ascontiguousarray(g1i[at[i]:at[i + 1]], dtype=np.uint8))
    (aq, ai), (bq, bi), (lqp, li), (hqp, hi), (icp, ici) = (cut(i) for i in range(5))
    if hi.any() or ici.any():
        raise ValueError("the trapdoor gives an infinite h_query or IC entry; take another seed")
    pk = Groth16ProvingKey(alpha_g1=g1s[0], beta_g1=g1s[1], delta_g1=g1s[2], beta_g2=g2s[0], delta_g2=g2s[2], a_query=aq, a_inf=ai, b_g1_query=bq, b_g1_inf=bi,
                           b_g2_query=g2s[3:].copy(), b_g2_inf=np.ascontiguousarray(g2i[3:], dtype=np.uint8), l_query=lqp, l_inf=li, h_query=hqp)
    vk = Groth16VerifyingKey(g1s[0].copy(), g2s[0].copy(), g2s[1].copy(), g2s[2].copy(), icp)
    r1cs = R1CS(log2_n, n_rows, m, l, csr_arrays(s["rows_a"]), csr_arrays(s["rows_b"]), csr_arrays(s["rows_c"]))
    wit = _rows([x for z in s["z"] for x in z]).reshape(n, m, 4) if n else np.zeros((0, m, 4), dtype=np.uint64)
    return r1cs, pk, vk, wit, s


FR_GENERATOR, FR_S = 7, 32      # r - 1 = 2^32 * odd, 7 generates Fr* (reference src/common.rs)


def fr_root_of_unity(log2_n):
    """the generator w of the 2^log2_n-point domain: 7^((r - 1) / 2^log2_n), i.e. (7^((r - 1) / 2^32))^(2^(32 - log2_n))"""
    if not 0 <= log2_n <= FR_S:
        raise ValueError("log2_n outside 0 .. 32")
    return pow(FR_GENERATOR, (R_ORDER - 1) >> log2_n, R_ORDER)


def bit_reverse(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def barycentric_eval(evals, z, log2_n, bitrev=False):
    """the polynomial of degree < N = 2^log2_n with p(w^i) = evals[i] (evals[i] belongs to w^bit_reverse(i) with bitrev) at z, on Python
    integers: (z^N - 1) / N * sum_i f_i w^i / (z - w^i), and f_i itself where z = w^i"""
    r, n = R_ORDER, 1 << log2_n
    if len(evals) != n:
        raise ValueError("evals hold %d values for N = %d" % (len(evals), n))
    w, z = fr_root_of_unity(log2_n), z % r
    dom = [1] * n
    for i in range(1, n):
        dom[i] = dom[i - 1] * w % r
    pts = [dom[bit_reverse(i, log2_n)] for i in range(n)] if bitrev else dom
    acc = 0
    for f, x in zip(evals, pts):
        if x == z:
            return int(f) % r
        acc += int(f) * x * pow(z - x, -1, r)
    return (pow(z, n, r) - 1) * pow(n, -1, r) * acc % r


def _kzg_points(engine, tau, cexp, pexp):
    n = len(cexp)
    g1s, inf = engine.g1_mul(G1_GENERATOR, _rows(list(cexp) + list(pexp)))
    tg2, _ = engine.g2_mul(G2_GENERATOR, _rows([tau]))
    setup = (G1_GENERATOR.copy(), G2_GENERATOR.copy(), tg2[0].copy())
    return setup, (g1s[:n].copy(), inf[:n].copy()), (g1s[n:].copy(), inf[n:].copy())


def kzg_instance(seed, n, bad=(), engine=None):
    """n synthetic KZG openings of one setup, built from secret exponents (Python integers mod r), no polynomial needed:
        setup   g1 = G1, g2 = G2, [tau] G2
        opening C_i = [c_i] G1, z_i, y_i random, pi_i = [(c_i - y_i) / (tau - z_i)] G1
    so that e(C_i - [y_i] g1 + [z_i] pi_i, g2) = e(pi_i, [tau] g2) holds by construction; the openings listed in `bad` get C + G1 and fail.
    -> (setup, commitments (n, 12), z (n, 4), y (n, 4), proofs (n, 12)), setup = (g1 (12,), g2 (24,), tau_g2 (24,))."""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    r = R_ORDER
    (tau,) = _ints(scalars(seed ^ 0x7A0, 1))
    c = _ints(scalars(seed ^ 0x0C, n))
    zw, yw = scalars(seed ^ 0x0D, n), scalars(seed ^ 0x0E, n)
    z, y = _ints(zw), _ints(yw)
    bad = set(int(i) for i in bad)
    pexp = [(c[i] - y[i]) * pow(tau - z[i], -1, r) % r for i in range(n)]
    cexp = [(c[i] + (1 if i in bad else 0)) % r for i in range(n)]
    setup, (cp, _), (pp, _) = _kzg_points(engine, tau, cexp, pexp)
    return setup, cp, zw, yw, pp


def kzg_blob_instance(seed, n, log2_n, bitrev=True, bad=(), engine=None):
    """n polynomials given by N = 2^log2_n random evaluations each (stored in bit-reversed order with bitrev, like blobs), their
    commitments [p_j(tau)] G1, a random point z_j each, y_j = p_j(z_j) and the proof [(p_j(tau) - y_j) / (tau - z_j)] G1 - the exponents by
    the barycentric formula on Python integers.  The polynomials listed in `bad` get C + G1.
    -> (setup, evals (n, N, 4), commitments (n, 12), z (n, 4), y (n, 4), proofs (n, 12))."""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    r, big_n = R_ORDER, 1 << log2_n
    (tau,) = _ints(scalars(seed ^ 0x7A1, 1))
    ew = scalars(seed ^ 0x0F, n * big_n).reshape(n, big_n, 4)
    zw = scalars(seed ^ 0x10, n)
    z = _ints(zw)
    bad = set(int(i) for i in bad)
    cexp, pexp, y = [], [], []
    for j in range(n):
        f = _ints(ew[j])
        pt, yj = barycentric_eval(f, tau, log2_n, bitrev), barycentric_eval(f, z[j], log2_n, bitrev)
        y.append(yj)
        cexp.append((pt + (1 if j in bad else 0)) % r)
        pexp.append((pt - yj) * pow(tau - z[j], -1, r) % r)
    setup, (cp, _), (pp, _) = _kzg_points(engine, tau, cexp, pexp)
    return setup, ew, cp, zw, _rows(y), pp


def kzg_cells_instance(seed, n, log2_n, log2_l, bad=(), engine=None):
    """n random polynomials of N = 2^log2_n coefficients with what the cell proofs need of a setup whose secret tau is derived from the
    seed: the monomial setup [tau^k] G1, k < N (its first l = 2^log2_l points are the verifier's), G2 and [tau^l] G2, and the commitments
    [f_j(tau)] G1 - the exponents on Python integers.  The polynomials listed in `bad` get C + G1.
    -> (monomial_g1 (N, 12), g2 (24,), tau_l_g2 (24,), coeffs (n, N, 4), commitments (n, 12))."""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    r, big_n = R_ORDER, 1 << log2_n
    (tau,) = _ints(scalars(seed ^ 0x7A2, 1))
    cw = scalars(seed ^ 0x11, n * big_n).reshape(n, big_n, 4)
    powers = [1] * big_n
    for k in range(1, big_n):
        powers[k] = powers[k - 1] * tau % r
    bad = set(int(i) for i in bad)
    cexp = [(sum(c * p for c, p in zip(_ints(cw[j]), powers)) + (1 if j in bad else 0)) % r for j in range(n)]
    g1s, _ = engine.g1_mul(G1_GENERATOR, _rows(powers + cexp))
    tg2, _ = engine.g2_mul(G2_GENERATOR, _rows([pow(tau, 1 << log2_l, r)]))
    return g1s[:big_n].copy(), G2_GENERATOR.copy(), tg2[0].copy(), cw, g1s[big_n:].copy()


def das_recover_instance(seed, n, log2_n, log2_l, bitrev=True, keep=None, engine=None):
    """n random blobs of N = 2^log2_n coefficients, extended to D = 2 N points, cut into M = D / l cells of l = 2^log2_l values (in the
    order bitrev names) and erased: every blob keeps `keep` cells drawn from the seed (M / 2 by default: a random half), the rows of the
    others are filled with 0xff bytes.  The cells come from the engine's fr_ntt.
    -> (values (n, M, l, 4), present (n, M) uint8, coeffs (n, N, 4): what das_recover must return)."""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    big_n, l = 1 << log2_n, 1 << log2_l
    big_d = 2 * big_n
    big_m = big_d // l
    keep = big_m // 2 if keep is None else int(keep)
    cw = scalars(seed ^ 0xDA5, n * big_n).reshape(n, big_n, 4)
    padded = np.zeros((n, big_d, 4), dtype=np.uint64)
    padded[:, :big_n] = cw
    ev = engine.fr_ntt(padded.reshape(-1, 4), log2_n + 1, bitrev=bitrev).reshape(n, big_d, 4) if n else padded
    values = ev.reshape(n, big_m, l, 4).copy() if bitrev else np.ascontiguousarray(ev.reshape(n, l, big_m, 4).transpose(0, 2, 1, 3))
    rng = np.random.RandomState((seed ^ 0xE7A5) & 0x7FFFFFFF)
    present = np.zeros((n, big_m), dtype=np.uint8)
    for j in range(n):
        present[j, rng.permutation(big_m)[:keep]] = 1
    values[present == 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return values, present, cw


def bls_instance(n, seed=SEED, engine=None, dst=b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"):
    """n valid BLS signatures from the seed: secret keys, messages of 0 .. 63 bytes, public keys [sk] g1 and signatures [sk] H(m), the
    hash and both multiplications on the engine.  -> (sks (n, 4), pks (n, 12), msgs (list of bytes), sigs (n, 24))"""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    sks = scalars(seed ^ 0xB15, n)
    raw = splitmix64(seed ^ 0x5E5, 9 * n).reshape(n, 9) if n else np.zeros((0, 9), dtype=np.uint64)
    msgs = [raw[i, 1:].tobytes()[:int(raw[i, 0]) % 64] for i in range(n)]
    if n == 0:
        return sks, np.zeros((0, 12), dtype=np.uint64), msgs, np.zeros((0, 24), dtype=np.uint64)
    pks, _ = engine.g1_mul(G1_GENERATOR, sks)
    h, _ = engine.hash_to_g2(msgs, dst)
    sigs, _ = engine.g2_mul(h, sks)
    return sks, pks, msgs, sigs


def bls_minsig_instance(n, same_key=False, seed=SEED, engine=None, dst=b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"):
    """n valid BLS signatures of the minimal-signature-size layout from the seed: secret keys (ONE key repeated when same_key), messages
    of 0 .. 63 bytes, public keys [sk] g2 and signatures [sk] H(m) in G1, the hash and both multiplications on the engine.
    -> (sks (n, 4), pks (n, 24), msgs (list of bytes), sigs (n, 12))"""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    sks = scalars(seed ^ 0xB16, n)
    if same_key and n:
        sks[:] = sks[0]
    raw = splitmix64(seed ^ 0x5E6, 9 * n).reshape(n, 9) if n else np.zeros((0, 9), dtype=np.uint64)
    msgs = [raw[i, 1:].tobytes()[:int(raw[i, 0]) % 64] for i in range(n)]
    if n == 0:
        return sks, np.zeros((0, 24), dtype=np.uint64), msgs, np.zeros((0, 12), dtype=np.uint64)
    pks, _ = engine.g2_mul(G2_GENERATOR, sks)
    h, _ = engine.hash_to_g1(msgs, dst)
    sigs, _ = engine.g1_mul(h, sks)
    return sks, pks, msgs, sigs


def bls_aggregate_instance(n_table, sizes, seed=SEED, engine=None, dst=b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"):
    """A table of n_table key pairs and one valid aggregate signature per committee size in `sizes`, from the seed: committee i draws
    sizes[i] rows (with repetition) and signs message i with the SUM of their secret keys, sig_i = [sum sk] H(m_i) - which is what the
    sum of the members' signatures is.  -> (sks (n_table, 4), table (n_table, 12), committees (list of lists), msgs, sigs (n, 24))"""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    n = len(sizes)
    sks = scalars(seed ^ 0xA66, n_table)
    table, _ = engine.g1_mul(G1_GENERATOR, sks) if n_table else (np.zeros((0, 12), dtype=np.uint64), None)
    draw = splitmix64(seed ^ 0xC0117, int(sum(sizes)))
    committees, at = [], 0
    for k in sizes:
        committees.append([int(v % np.uint64(n_table)) for v in draw[at:at + k]])
        at += k
    raw = splitmix64(seed ^ 0x5E5A, 9 * n).reshape(n, 9) if n else np.zeros((0, 9), dtype=np.uint64)
    msgs = [raw[i, 1:].tobytes()[:int(raw[i, 0]) % 64] for i in range(n)]
    if n == 0:
        return sks, table, committees, msgs, np.zeros((0, 24), dtype=np.uint64)
    sums = np.stack([int_to_scalar(sum(scalar_to_int(sks[r]) for r in c) % R_ORDER) for c in committees])
    h, _ = engine.hash_to_g2(msgs, dst)
    sigs, inf = engine.g2_mul(h, sums)
    sigs[inf != 0] = 0
    sigs[inf != 0, 12] = 1
    return sks, table, committees, msgs, sigs


def bls_minsig_aggregate_instance(n_table, sizes, seed=SEED, engine=None, dst=b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_POP_"):
    """bls_aggregate_instance in the minimal-signature-size layout: a table of n_table keys [sk] g2 and one valid aggregate signature in
    G1 per committee size, sig_i = [sum sk] H(m_i).  -> (sks (n_table, 4), table (n_table, 24), committees (list of lists), msgs,
    sigs (n, 12))"""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    n = len(sizes)
    sks = scalars(seed ^ 0xA67, n_table)
    table, _ = engine.g2_mul(G2_GENERATOR, sks) if n_table else (np.zeros((0, 24), dtype=np.uint64), None)
    draw = splitmix64(seed ^ 0xC0118, int(sum(sizes)))
    committees, at = [], 0
    for k in sizes:
        committees.append([int(v % np.uint64(n_table)) for v in draw[at:at + k]])
        at += k
    raw = splitmix64(seed ^ 0x5E5B, 9 * n).reshape(n, 9) if n else np.zeros((0, 9), dtype=np.uint64)
    msgs = [raw[i, 1:].tobytes()[:int(raw[i, 0]) % 64] for i in range(n)]
    if n == 0:
        return sks, table, committees, msgs, np.zeros((0, 12), dtype=np.uint64)
    sums = np.stack([int_to_scalar(sum(scalar_to_int(sks[r]) for r in c) % R_ORDER) for c in committees])
    h, _ = engine.hash_to_g1(msgs, dst)
    sigs, inf = engine.g1_mul(h, sums)
    sigs[inf != 0] = 0
    sigs[inf != 0, 6] = 1
    return sks, table, committees, msgs, sigs


def bls_aggregate_verify_instance(sizes, seed=SEED, engine=None, dst=b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"):
    """n = len(sizes) valid aggregate signatures for AggregateVerify from the seed: signature j is the sum of sizes[j] individual
    signatures [sk_i] H(m_i) by distinct keys on distinct messages (the message's number leads), summed by g2_segment_sum.
    -> (sks (n_msg, 4), pks (n_msg, 12), msgs (list of n_msg bytes), seg_off uint64 (n + 1,), sigs (n, 24))"""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    n, n_msg = len(sizes), int(sum(sizes))
    sks = scalars(seed ^ 0xA6B, n_msg)
    raw = splitmix64(seed ^ 0x5E5C, 9 * n_msg).reshape(n_msg, 9) if n_msg else np.zeros((0, 9), dtype=np.uint64)
    msgs = [int(i).to_bytes(4, "little") + raw[i, 1:].tobytes()[:int(raw[i, 0]) % 64] for i in range(n_msg)]
    seg_off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        seg_off[1:] = np.cumsum(sizes, dtype=np.uint64)
    if n_msg == 0:
        sigs = np.zeros((n, 24), dtype=np.uint64)
        sigs[:, 12] = 1
        return sks, np.zeros((0, 12), dtype=np.uint64), msgs, seg_off, sigs
    pks, _ = engine.g1_mul(G1_GENERATOR, sks)
    h, _ = engine.hash_to_g2(msgs, dst)
    each, _ = engine.g2_mul(h, sks)
    sigs, _, _ = engine.g2_segment_sum(each, np.arange(n_msg, dtype=np.uint32), seg_off)
    return sks, pks, msgs, seg_off, sigs


def bls_grouped_instance(sizes, seed=SEED, engine=None, dst=b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"):
    """n = sum(sizes) valid BLS signatures ORDERED BY MESSAGE over m = len(sizes) distinct messages, from the seed: group g holds sizes[g]
    signatures of message g (a size may be 0: a message nobody signed), sig_i = [sk_i] H(m_g).  The messages are 4 to 67 bytes and
    pairwise distinct (the group's number leads).  -> (sks (n, 4), pks (n, 12), msgs (list of m bytes), grp_off uint64 (m + 1,), sigs (n, 24))"""
    if engine is None:
        from .pairings import default_engine
        engine = default_engine()
    m, n = len(sizes), int(sum(sizes))
    sks = scalars(seed ^ 0x6B15, n)
    raw = splitmix64(seed ^ 0x65E5, 9 * m).reshape(m, 9) if m else np.zeros((0, 9), dtype=np.uint64)
    msgs = [int(g).to_bytes(4, "little") + raw[g, 1:].tobytes()[:int(raw[g, 0]) % 64] for g in range(m)]
    grp_off = np.zeros(m + 1, dtype=np.uint64)
    if m:
        grp_off[1:] = np.cumsum(sizes, dtype=np.uint64)
    if n == 0:
        return sks, np.zeros((0, 12), dtype=np.uint64), msgs, grp_off, np.zeros((0, 24), dtype=np.uint64)
    pks, _ = engine.g1_mul(G1_GENERATOR, sks)
    h, _ = engine.hash_to_g2(msgs, dst)
    sigs, _ = engine.g2_mul(np.repeat(h, np.asarray(sizes, dtype=np.int64), axis=0), sks)
    return sks, pks, msgs, grp_off, sigs
