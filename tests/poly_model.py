"""The NTT over the BLS12-381 scalar field on Python integers: the model the device transform (zkp_fr_ntt_batch) and the host replay of
its schedule (tests/poly_plan_check.cpp) are compared with, byte for byte.  Nothing here imports the library under test.

forward:  out[i] = sum_k in[k] (s w^i)^k mod r, w = 7^((r - 1) / N), s = 7 with `coset` else 1; with `bitrev` slot i holds the value
          at s w^bitrev(i)
inverse:  the exact inverse map under the same other flags"""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
GENERATOR = 7
INVERSE, BITREV, COSET = 1, 2, 4


def root_of_unity(log2_n):
    return pow(GENERATOR, (R - 1) >> log2_n, R)


def bit_reverse(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def domain(log2_n, inverse=False):
    """w^i (or w^-i) for i < N"""
    w = root_of_unity(log2_n)
    if inverse:
        w = pow(w, -1, R)
    out, acc = [], 1
    for _ in range(1 << log2_n):
        out.append(acc)
        acc = acc * w % R
    return out


def _dif(a, log2_n, dom):
    """natural order in, bit-reversed order out, in place"""
    n = 1 << log2_n
    half = n >> 1
    step = 1
    while half:
        for start in range(0, n, 2 * half):
            for j in range(half):
                x, y = a[start + j], a[start + j + half]
                a[start + j] = (x + y) % R
                a[start + j + half] = (x - y) * dom[j * step] % R
        half >>= 1
        step <<= 1


def _dit(a, log2_n, dom):
    """bit-reversed order in, natural order out, in place"""
    n = 1 << log2_n
    half = 1
    step = n >> 1
    while half < n:
        for start in range(0, n, 2 * half):
            for j in range(half):
                x, y = a[start + j], a[start + j + half] * dom[j * step] % R
                a[start + j] = (x + y) % R
                a[start + j + half] = (x - y) % R
        half <<= 1
        step >>= 1


def ntt(vals, log2_n, inverse=False, bitrev=False, coset=False):
    n = 1 << log2_n
    assert len(vals) == n
    rev = [bit_reverse(i, log2_n) for i in range(n)]
    if not inverse:
        a = list(vals)
        if coset:
            s = 1
            for k in range(n):
                a[k] = a[k] * s % R
                s = s * GENERATOR % R
        _dif(a, log2_n, domain(log2_n))
        return a if bitrev else [a[rev[i]] for i in range(n)]
    a = list(vals) if bitrev else [vals[rev[i]] for i in range(n)]
    _dit(a, log2_n, domain(log2_n, inverse=True))
    scale = pow(n, -1, R)
    step = pow(GENERATOR, -1, R) if coset else 1
    for k in range(n):
        a[k] = a[k] * scale % R
        scale = scale * step % R
    return a


def ntt_flags(vals, log2_n, flags):
    return ntt(vals, log2_n, bool(flags & INVERSE), bool(flags & BITREV), bool(flags & COSET))


def ntt_definition(vals, log2_n, bitrev=False, coset=False):
    """the forward transform straight from its definition, O(N^2)"""
    n = 1 << log2_n
    w = root_of_unity(log2_n)
    s = GENERATOR if coset else 1
    out = []
    for i in range(n):
        x = s * pow(w, bit_reverse(i, log2_n) if bitrev else i, R) % R
        acc = 0
        for c in reversed(vals):
            acc = (acc * x + c) % R
        out.append(acc)
    return out


def to_bytes(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def from_bytes(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
