"""CPU gate for the scalar field: csrc/zkp_fr.hpp - the text the GPU kernels compile - built for the host with g++ and compared with
Python integers: the derived constants against pow / %, every operation on edge operands, Montgomery pre-images, the reference's own
test operands (tests/golden/fr_operands.json: inputs only) and seeded random values, the wide reduction, and the fold's accumulator
at its bound."""
import json
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm_pairings_amd", "csrc")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MONT = 1 << 256

HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "zkp_fr.hpp"
using namespace zkp::fr;
static void put(const uint32_t* v, int n) { for (int i = n - 1; i >= 0; i--) std::printf("%08x", v[i]); std::printf("\n"); }
static void get(const char* hex, uint32_t* v, int n) {
    const size_t len = std::strlen(hex);
    for (int i = 0; i < n; i++) {
        char buf[9] = "00000000";
        for (int k = 0; k < 8; k++) {
            const long at = (long)len - 8 * (i + 1) + k;
            if (at >= 0) buf[k] = hex[at];
        }
        v[i] = (uint32_t)std::strtoul(buf, nullptr, 16);
    }
}
int main() {
    char op[16], ha[160], hb[160];
    while (std::scanf("%15s %159s %159s", op, ha, hb) == 3) {
        uint32_t a[ACC_WORDS], b[ACC_WORDS], r[ACC_WORDS];
        if (!std::strcmp(op, "consts")) {
            constexpr Consts K = make_consts();
            put(K.r, NW); put(K.rm2, NW); put(K.one, NW); put(K.r2, NW); put(K.r3, NW); put(K.r4, NW); std::printf("%08x\n", K.inv);
            continue;
        }
        if (!std::strcmp(op, "wide")) {          // a: 17 words -> mod r
            get(ha, a, ACC_WORDS);
            reduce_wide(r, a);
            put(r, NW);
            continue;
        }
        if (!std::strcmp(op, "acc")) {           // a: the number of terms, b: the operand: n times acc += b b, then the raw words and the reduction
            const unsigned long n = std::strtoul(ha, nullptr, 10);
            get(hb, b, NW);
            for (int i = 0; i < ACC_WORDS; i++) a[i] = 0;
            for (unsigned long i = 0; i < n; i++) acc_mad(a, b, b);
            put(a, ACC_WORDS);
            reduce_wide(r, a);
            put(r, NW);
            continue;
        }
        if (!std::strcmp(op, "accsum")) {        // a: 17 words, b: 17 words -> a + b through acc_add
            get(ha, a, ACC_WORDS); get(hb, b, ACC_WORDS);
            acc_add(a, b, ACC_WORDS);
            put(a, ACC_WORDS);
            continue;
        }
        get(ha, a, NW); get(hb, b, NW);
        if (!std::strcmp(op, "mul")) mul(r, a, b);
        else if (!std::strcmp(op, "add")) add(r, a, b);
        else if (!std::strcmp(op, "sub")) sub(r, a, b);
        else if (!std::strcmp(op, "neg")) neg(r, a);
        else if (!std::strcmp(op, "square")) mul(r, a, a);
        else if (!std::strcmp(op, "invert")) invert(r, a);
        else if (!std::strcmp(op, "montmul")) mont_mul(r, a, b);
        else if (!std::strcmp(op, "canon")) { std::printf("%d\n", is_canonical(a) ? 1 : 0); continue; }
        else return 2;
        put(r, NW);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def fr_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("fr")
    src = d / "fr_harness.cpp"
    src.write_text(HARNESS)
    exe = str(d / "fr_harness")
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
                         str(src)], capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    return exe


def _run(exe, lines, timeout=600):
    out = subprocess.run([exe], input="".join("%s %s %s\n" % (o, a, b) for o, a, b in lines), capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split()


def _h(v):
    return "%x" % v


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "fr_operands.json")) as f:
        return json.load(f)


def _operands():
    g = _golden()
    edge = {0, 1, 2, R - 1, R - 2}
    for k in range(1, 255):
        edge |= {1 << k, (1 << k) - 1, R - (1 << k)}
    edge = {v for v in edge if 0 <= v < R}
    rinv = pow(MONT, -1, R)
    pre = {v * rinv % R for v in edge} | {v * MONT % R for v in edge}          # what the edge values are the Montgomery forms of, and their forms
    ref = {int(g["largest"], 16), int(g["fr_r"], 16), int(g["fr_r2"], 16), int(g["fr_r3"], 16)}
    rng = random.Random(0xF2)
    return sorted(edge), sorted(pre), sorted(ref), [rng.randrange(R) for _ in range(3000)]


def test_derived_constants_match_python_integers(fr_exe):
    out = _run(fr_exe, [("consts", "0", "0")])
    r, rm2, one, r2, r3, r4 = (int(x, 16) for x in out[:6])
    inv = int(out[6], 16)
    assert r == R and rm2 == R - 2
    assert one == MONT % R and r2 == pow(MONT, 2, R) and r3 == pow(MONT, 3, R) and r4 == pow(MONT, 4, R)
    assert inv == (-pow(R, -1, 1 << 32)) % (1 << 32)
    g = _golden()   # and the reference lists the same R, R^2, R^3
    assert one == int(g["fr_r"], 16) and r2 == int(g["fr_r2"], 16) and r3 == int(g["fr_r3"], 16) and int(g["largest"], 16) == R - 1


def test_every_operation_against_python_integers(fr_exe):
    edge, pre, ref, rnd = _operands()
    small = [0, 1, 2, R - 1, R - 2, 1 << 32, (1 << 32) - 1, 1 << 64, (1 << 128) - 1, 1 << 254, R - (1 << 200)] + ref
    pairs = [(a, b) for a in small for b in small]
    special = edge + pre + ref
    rng = random.Random(0xF3)
    pairs += [(a, rng.choice(special)) for a in special] + [(rng.choice(special), b) for b in rnd[:500]] + list(zip(rnd[0::2], rnd[1::2]))
    lines, want = [], []
    for a, b in pairs:
        for op, v in (("mul", a * b % R), ("add", (a + b) % R), ("sub", (a - b) % R)):
            lines.append((op, _h(a), _h(b)))
            want.append(v)
    unary = special + rnd
    for a in unary:
        for op, v in (("neg", -a % R), ("square", a * a % R)):
            lines.append((op, _h(a), "0"))
            want.append(v)
    for a in small + ref + pre[:40] + rnd[:200]:
        lines.append(("invert", _h(a), "0"))
        want.append(pow(a, R - 2, R))                       # 0 for 0
    got = [int(x, 16) for x in _run(fr_exe, lines)]
    assert len(got) == len(want)
    bad = [(lines[i], got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:3]


def test_invert_is_the_inverse_and_zero_for_zero(fr_exe):
    _, _, ref, rnd = _operands()
    vals = [1, 2, R - 1] + ref + rnd[:50]
    inv = [int(x, 16) for x in _run(fr_exe, [("invert", _h(a), "0") for a in vals])]
    assert all(a * i % R == 1 for a, i in zip(vals, inv))
    assert _run(fr_exe, [("invert", "0", "0")]) == ["0" * 64]


def test_montgomery_product_takes_any_256_bit_left_operand(fr_exe):
    """the wide reduction feeds raw 256-bit words into mont_mul: a < 2^256 (not < r) against b < r"""
    rng = random.Random(0xF4)
    a_s = [MONT - 1, MONT - 2, R, R + 1, 2 * R, 2 * R + 1, MONT - R] + [rng.getrandbits(256) for _ in range(500)]
    b_s = [R - 1, 1, 0, pow(MONT, 2, R)] + [rng.randrange(R) for _ in range(20)]
    rinv = pow(MONT, -1, R)
    lines = [("montmul", _h(a), _h(b)) for a in a_s for b in b_s]
    got = [int(x, 16) for x in _run(fr_exe, lines)]
    assert got == [a * b * rinv % R for a in a_s for b in b_s]


def test_is_canonical(fr_exe):
    vals = [0, 1, R - 1, R, R + 1, MONT - 1, 1 << 255, R - (1 << 32), R + (1 << 32)]
    assert _run(fr_exe, [("canon", _h(v), "0") for v in vals]) == ["1" if v < R else "0" for v in vals]


def test_wide_reduction_against_python_integers(fr_exe):
    g = _golden()
    rng = random.Random(0xF5)
    vals = [int(v, 16) for v in g["from_u512"]] + [int.from_bytes(bytes(b), "little") for b in g["from_bytes_wide"]]
    want_ref = [0, 1, MONT % R, R - 1]                      # what the reference's tests expect of its four inputs
    vals += [0, 1, R, R - 1, MONT - 1, MONT, (1 << 512) - 1, 1 << 512, (1 << 544) - 1, (R - 1) ** 2, (1 << 24) * (R - 1) ** 2, (1 << 534) - 1]
    vals += [rng.getrandbits(512) for _ in range(1000)] + [rng.getrandbits(544) for _ in range(1000)] + [rng.getrandbits(534) for _ in range(200)]
    got = [int(x, 16) for x in _run(fr_exe, [("wide", _h(v), "0") for v in vals])]
    assert got == [v % R for v in vals]
    assert got[:4] == want_ref


def test_the_accumulator_bound_by_arithmetic():
    """2^24 products of canonical operands stay below 2^534, of ANY 256-bit operands below 2^544 = 17 words"""
    n = 1 << 24
    assert n * (R - 1) ** 2 < 1 << 534 and (R - 1) ** 2 < 1 << 510
    assert n * (MONT - 1) ** 2 < 1 << (32 * 17)


def test_the_accumulator_is_exact_at_the_largest_terms(fr_exe):
    """n terms of (r - 1)(r - 1), no reduction in between: the 17 words are the integer n (r - 1)^2, its reduction is n mod r; partial
    accumulators join exactly"""
    n = 1 << 20                                             # the largest count a host run takes in seconds
    out = _run(fr_exe, [("acc", str(n), _h(R - 1)), ("acc", "3", _h(MONT - 1))])
    assert int(out[0], 16) == n * (R - 1) ** 2 and int(out[1], 16) == n % R
    assert int(out[2], 16) == 3 * (MONT - 1) ** 2 and int(out[3], 16) == 3 * (MONT - 1) ** 2 % R
    # 16 partial sums of 2^20 such terms each are what 2^24 terms leave behind: joined by acc_add they give the bound's integer
    part = n * (R - 1) ** 2
    acc = 0
    for _ in range(16):
        acc = int(_run(fr_exe, [("accsum", _h(acc), _h(part))])[0], 16)
    assert acc == (1 << 24) * (R - 1) ** 2
    assert int(_run(fr_exe, [("wide", _h(acc), "0")])[0], 16) == (1 << 24) % R
