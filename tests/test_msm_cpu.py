"""CPU gate for group addition and the bucket MSM: the new entry points are exported and bound, a Python model of the signed-digit
decomposition (k_msm_digits) gives back every scalar exactly, the MSM planner (csrc/zkp_msm_plan.hpp) keeps every per-launch count in
32 bits at the ABI maxima under ASan and UBSan, the GPU tests' shape table (tests/msm_shapes.py) reaches the plans it claims, and the
new kernels neither spill nor use scratch in the built code object."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
EDGE = [0, 1, 2, R - 1, R, 1 << 255, (1 << 256) - 1, 0x5555 << 240, (1 << 256) - (1 << 128)]
NEW = ["zkp_g1_add_batch", "zkp_g2_add_batch", "zkp_g1_msm_batch", "zkp_g2_msm_batch", "zkp_g1_add_batch_dev", "zkp_g2_add_batch_dev",
       "zkp_g1_msm_batch_dev", "zkp_g2_msm_batch_dev", "zkp_msm_profile_dev"]


def test_new_symbols_are_exported_and_bound():
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.zkp_abi_version() == 4


def test_bad_sizes_are_refused_without_a_device():
    from zkvm_pairings_amd import _lib
    lib = _lib.load()
    # a null context is refused before anything else
    assert lib.zkp_g1_msm_batch(None, None, None, None, 1, 1, 0, None, None) == -1
    assert lib.zkp_g2_add_batch(None, None, None, None, None, 1, None, None) == -1


def digits(k, c):
    """model of k_msm_digits: W = 256/c + 1 signed digits, d in [-2^(c-1) + 1, 2^(c-1)]"""
    half, carry, out = 1 << (c - 1), 0, []
    for w in range(256 // c + 1):
        d = ((k >> (w * c)) & ((1 << c) - 1)) + carry
        carry = 1 if d > half else 0
        d -= carry << c
        out.append(d)
    assert carry == 0
    return out


@pytest.mark.parametrize("c", range(2, 17))
def test_signed_digits_reproduce_every_scalar(c):
    import random
    rng = random.Random(c)
    for k in EDGE + [rng.getrandbits(256) for _ in range(200)]:
        ds = digits(k, c)
        assert all(-(1 << (c - 1)) < d <= (1 << (c - 1)) for d in ds)
        assert sum(d << (c * w) for w, d in enumerate(ds)) == k


PLAN_CHECK = r"""
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <initializer_list>
#include "zkp_msm_plan.hpp"
using namespace zkp::msm;
static int fails = 0;
#define REQ(x) do { if (!(x)) { std::printf("FAIL %s m=%zu n=%zu sh=%d\n", #x, m, n, (int)sh); fails++; return; } } while (0)
static const uint64_t U32 = 0xffffffffull, I32 = 0x7fffffffull;
static void check(size_t m, size_t n, bool sh) {
    Plan p;
    REQ(make_plan(m, n, sh, &p));
    const uint64_t W = p.windows, nb = p.nb;
    REQ(p.c >= 2 && p.c <= 16 && W == 256 / p.c + 1 && nb == (1ull << (p.c - 1)));
    REQ((uint64_t)p.segs * p.passes >= n && (uint64_t)p.segs * (p.passes - 1) < n && p.segs >= 1);
    REQ((uint64_t)p.terms == (uint64_t)p.segs * m && (uint64_t)p.keys == (uint64_t)p.terms * W && p.keys <= I32);   // the sort's int count
    REQ((uint64_t)p.buckets == (uint64_t)p.segs * W * nb && p.buckets <= MAX_BUCKETS);
    REQ(p.key_bits <= 31 && (uint64_t)p.buckets < (1ull << p.key_bits));                 // KEY_NONE's low bits above every bucket id
    REQ((((uint64_t)p.segs * W) << (p.c - 1)) <= U32);                                   // (seg W + w) << (c - 1) in 32 bits
    REQ((uint64_t)p.split * p.chunk == nb && (uint64_t)p.sums == (uint64_t)p.segs * W);
    REQ((uint64_t)p.sums * p.split * 2 <= U32 && (uint64_t)p.segs * 2 <= U32);         // reduce / final lanes (G2: pairs)
    REQ(p.levels >= 1 && p.levels <= MAX_LEVELS && p.wlevels >= 1 && p.wlevels <= MAX_LEVELS);
    REQ(p.level_in[0] == p.keys && p.wlevel_in[0] == p.sums * p.split);
    for (int l = 0; l < p.levels; l++) {
        REQ((uint64_t)runs_of(p.level_in[l]) * 2 * 64 <= U32);                         // G2 lanes, rounded up to whole blocks
        REQ(2ull * runs_of(p.level_in[l]) <= p.part_cap[l & 1]);                       // the level's output slots fit its buffer
        REQ(l + 1 == p.levels ? p.level_in[l] <= RUN : p.level_in[l + 1] == 2 * runs_of(p.level_in[l]));
    }
    for (int l = 0; l < p.wlevels; l++) REQ(2ull * runs_of(p.wlevel_in[l]) <= p.part_cap[l & 1]);
    REQ((uint64_t)p.pts * 4 <= U32 && (uint64_t)p.terms <= (1ull << 24));             // Fp records, point indices below bit 31
    for (uint32_t np = 2; np <= 4; np += 2) {
        const Layout L = make_layout(p, np, 1 << 20);
        REQ(L.pts < L.keys_in && L.keys_in < L.vals_in && L.vals_in < L.keys_out && L.keys_out < L.vals_out && L.vals_out < L.sort_temp);
        REQ(L.sort_temp < L.buckets && L.buckets < L.part_k[0] && L.part_j[1] < L.chunk_k && L.chunk_j < L.wsums && L.wsums < L.total);
    }
}
int main() {
    size_t ms[64];
    int k = 0;
    for (int b = 0; b <= 24; b++) ms[k++] = (size_t)1 << b;
    const size_t extra[] = {3, 7, 63, 65, 1000, 4097, 65535, 65537, 1000003, (1u << 24) - 1, (1u << 23) + 1};
    for (size_t e : extra) ms[k++] = e;
    for (int i = 0; i < k; i++) {
        const size_t m = ms[i], top = MAX_TERMS / m;
        const size_t ns[] = {1, 2, 5, 300, top / 2 ? top / 2 : 1, top - 1 ? top - 1 : 1, top};
        for (size_t n : ns)
            for (int sh = 0; sh < 2 && n <= top; sh++) check(m, n, sh != 0);
    }
    {
        Plan p;
        if (make_plan(1, MAX_TERMS + 1, false, &p) || !msm_args_bad(1, MAX_TERMS + 1) || !msm_args_bad(0, 1) || !msm_args_bad(MAX_TERMS + 1, 1) ||
            msm_args_bad(0, 0) || msm_args_bad(1, MAX_TERMS) || msm_args_bad(MAX_TERMS, 1)) {
            std::printf("FAIL the ABI limits\n");
            fails++;
        }
    }
    for (size_t m : {(size_t)1 << 10, (size_t)1 << 14, (size_t)1 << 20, (size_t)1 << 24}) {
        Plan p;
        make_plan(m, 1, false, &p);
        const Layout a = make_layout(p, 2, 0), b = make_layout(p, 4, 0);
        std::printf("bytes per term at m=%zu (c=%u): G1 %.0f G2 %.0f\n", m, p.c, (double)a.total / m, (double)b.total / m);
    }
    if (fails) return 1;
    std::printf("msm plan_check ok\n");
    return 0;
}
"""


def test_msm_planner_under_asan_and_ubsan_at_the_abi_maxima(tmp_path):
    src = tmp_path / "msm_plan_check.cpp"
    src.write_text(PLAN_CHECK)
    exe = str(tmp_path / "msm_plan_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                         "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "zkvm_pairings_amd", "csrc"), "-o", exe, str(src)],
                        capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "msm plan_check ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    with open(os.path.join(ROOT, "zkvm_pairings_amd", "csrc", "zkp_msm.hip")) as f:
        assert '#include "zkp_msm_plan.hpp"' in f.read()


SHAPE_PLAN = r"""
#include <cstdio>
#include "zkp_msm_plan.hpp"
using namespace zkp::msm;
int main() {
    size_t m, n;
    int sh;
    while (std::scanf("%zu %zu %d", &m, &n, &sh) == 3) {
        Plan p;
        const int ok = make_plan(m, n, sh != 0, &p) ? 1 : 0;
        std::printf("%d %u %u %u %u %d %u %u %u\n", ok, p.c, p.passes, p.split, p.chunk, p.levels, p.segs, m > 1 ? choose_c(m - 1) : 0u,
                    m < MAX_TERMS ? choose_c(m + 1) : 0u);
    }
    return 0;
}
"""


def test_msm_shape_table_reaches_the_plans_it_claims(tmp_path):
    """tests/msm_shapes.py lists the shapes the GPU MSM tests run; make_plan must give each row exactly its fields, and the rows
    together must cover every window width for G1 and G2, both ends of every c range for G1, passes >= 3 with a partial last pass
    (shared and not), split 1 with chunk > 1, and the largest admitted call"""
    import msm_shapes as ms
    src = tmp_path / "msm_shape_plan.cpp"
    src.write_text(SHAPE_PLAN)
    exe = str(tmp_path / "msm_shape_plan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "zkvm_pairings_amd", "csrc"), "-o", exe,
                         str(src)], capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    rows = ms.ALL
    feed = "".join("%d %d %d\n" % (s.m, s.n_msm, int(s.shared)) for s in rows)
    out = subprocess.run([exe], input=feed, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.split("\n")[:len(rows)]
    assert len(lines) == len(rows)
    ends = {}
    for s, line in zip(rows, lines):
        ok, c, passes, split, chunk, levels, segs, c_prev, c_next = map(int, line.split())
        assert ok == 1 and s.m * s.n_msm <= ms.MAX_TERMS, s
        assert (c, passes, split, chunk, levels, segs) == (s.c, s.passes, s.split, s.chunk, s.levels, s.segs), (s, line)
        if s.passes > 1:
            assert s.n_msm % segs != 0, s                               # the last pass is partial
        if 1 in s.groups:
            ends.setdefault(c, set())
            if c_prev != c:
                ends[c].add("low")
            if c_next != c:
                ends[c].add("high")
    for which in (1, 2):
        assert {s.c for s in rows if which in s.groups} == set(range(2, 17)), which
    assert all(ends.get(c) == {"low", "high"} for c in range(2, 17)), ends
    multi = [s for s in rows if s.passes >= 3]
    assert {s.shared for s in multi} == {False, True}
    assert any(s.split == 1 and s.chunk > 1 for s in rows)
    assert any(s.m * s.n_msm == ms.MAX_TERMS and 1 in s.groups for s in rows)
    assert {s.split for s in rows if s.chunk > 1} >= {1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024}


def _kernels():
    data = open(SO, "rb").read()
    out = {}
    for i in [m.start() for m in re.finditer(b"\x7fELF\x02\x01\x01", data)][1:]:
        path = "/tmp/zkp_msm_codeobject_%d_%d.elf" % (os.getpid(), i)
        with open(path, "wb") as f:
            f.write(data[i:])
        notes = subprocess.run([READELF, "--notes", path], capture_output=True, text=True).stdout
        os.unlink(path)
        for blk in notes.split("- .agpr_count")[1:]:
            nm = re.search(r"\.name:\s+(\S+)", blk)
            if nm:
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                out[nm.group(1)] = {"spill": g("vgpr_spill_count"), "scratch": g("private_segment_fixed_size")}
    return out


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="library not built / no llvm-readelf")
def test_new_kernels_do_not_spill():
    k = _kernels()
    new = {n: v for n, v in k.items() if "k_add28" in n or "k_msm_" in n}
    assert len(new) == 2 + 2 + 4 + 2 + 2, sorted(new)          # add G1/G2, points + digits, accum x4, reduce x2, final x2
    for n, v in new.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (n, v)
    for bad in ("6k_coopILi", "5k_ksqE", "k_prep_linesILb1E"):
        assert not any(bad in n for n in new)
