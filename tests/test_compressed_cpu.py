"""CPU gate of the compressed point format: the Python model (tests/compressed_model.py) against the known answers and the curve
model, the Fp2 square-root route the decompression kernel takes, and the C boundary (the header declares the twelve new entry
points and the built library exports them).  No GPU needed."""
import os
import random
import re

import pytest

import bls12_381_model as m
import compressed_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = m.P

G1_KAT = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
G2_KAT = bytes.fromhex("93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                       "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")
NEW_SYMBOLS = ["zkp_fp_sqrt_batch", "zkp_fp2_sqrt_batch", "zkp_g1_decompress_batch", "zkp_g2_decompress_batch", "zkp_g1_compress_batch",
               "zkp_g2_compress_batch", "zkp_g1_decompress_batch_dev", "zkp_g2_decompress_batch_dev", "zkp_g1_compress_batch_dev",
               "zkp_g2_compress_batch_dev", "zkp_points_check_compressed_batch", "zkp_points_check_compressed_batch_dev"]


def test_generator_kats_decode_to_the_generators():
    assert cm.g1_decompress(G1_KAT) == (0, m.G1_GEN)
    assert cm.g2_decompress(G2_KAT) == (0, m.G2_GEN)
    assert cm.g1_compress(m.G1_GEN) == G1_KAT and cm.g2_compress(m.G2_GEN) == G2_KAT


def test_negated_generators_carry_the_sort_flag():
    n1, n2 = m.g1_neg(m.G1_GEN), m.g2_neg(m.G2_GEN)
    b1, b2 = cm.g1_compress(n1), cm.g2_compress(n2)
    assert b1[0] & 0x20 and b2[0] & 0x20
    assert b1 == bytes([G1_KAT[0] | 0x20]) + G1_KAT[1:] and b2 == bytes([G2_KAT[0] | 0x20]) + G2_KAT[1:]
    assert cm.g1_decompress(b1) == (0, n1) and cm.g2_decompress(b2) == (0, n2)


def test_infinity_and_malformed_flags():
    assert cm.g1_compress(None) == bytes([0xC0]) + bytes(47)
    assert cm.g1_decompress(bytes([0xC0]) + bytes(47)) == (0, None)
    assert cm.g2_decompress(bytes([0xC0]) + bytes(95)) == (0, None)
    assert cm.g1_decompress(bytes([0xE0]) + bytes(47))[0] == 2               # infinity with the sort flag
    assert cm.g1_decompress(bytes([0xC0]) + bytes(46) + b"\x01")[0] == 2     # infinity over non-zero bytes
    assert cm.g1_decompress(bytes([G1_KAT[0] & 0x7F]) + G1_KAT[1:])[0] == 2  # compression flag missing
    assert cm.g1_decompress(bytes([0x80 | 0x1A]) + bytes(47))[0] in (0, 3)   # a small finite x: a point or no root
    big = bytearray((P + 5).to_bytes(48, "big"))
    big[0] |= 0x80
    assert cm.g1_decompress(bytes(big))[0] == 1
    assert cm.g2_decompress(bytes(big) + bytes(48))[0] == 1                   # x.c1 >= p
    assert cm.g2_decompress(bytes([0x80]) + bytes(47) + (P + 5).to_bytes(48, "big"))[0] == 1   # x.c0 >= p


def test_model_round_trip_on_model_points():
    rng = random.Random(0x5EC)
    for _ in range(12):
        k = rng.randrange(1, m.R_ORDER)
        p1, p2 = m.g1_mul(m.G1_GEN, k), m.g2_mul(m.G2_GEN, k)
        assert cm.g1_decompress(cm.g1_compress(p1)) == (0, p1)
        assert cm.g2_decompress(cm.g2_compress(p2)) == (0, p2)
        n1, n2 = m.g1_neg(p1), m.g2_neg(p2)
        assert cm.g1_decompress(cm.g1_compress(n1)) == (0, n1)
        assert cm.g2_decompress(cm.g2_compress(n2)) == (0, n2)


def test_fp2_sqrt_route_of_the_kernel():
    """the decompression kernel's Fp2 root (norm root, then t^((p-3)/4)): squares give a root, non-squares none, a1 = 0 both ways"""
    rng = random.Random(0xF2)
    squares = nonsquares = 0
    for i in range(600):
        a = (rng.randrange(P), rng.randrange(P))
        if i % 3 == 0:
            a = m.f2_sqr(a)
        if i % 50 == 1:
            a = (a[0], 0)
        r = cm.fp2_sqrt_fast(a)
        norm_is_square = pow((a[0] * a[0] + a[1] * a[1]) % P, (P - 1) // 2, P) in (0, 1)
        if r is None:
            nonsquares += 1
            assert not norm_is_square
        else:
            squares += 1
            assert m.f2_sqr(r) == (a[0] % P, a[1] % P)
    for a0 in (0, 1, 4, P - 1, P - 4, 3):          # a1 = 0: sqrt(a0) or u sqrt(-a0), both always exist
        r = cm.fp2_sqrt_fast((a0, 0))
        assert r is not None and m.f2_sqr(r) == (a0, 0)
    assert squares > 150 and nonsquares > 150


def _declared():
    with open(os.path.join(ROOT, "include", "zkp_pairings.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(zkp_[a-z0-9_]+)\s*\(", text))


def test_header_declares_and_library_exports_the_compressed_entry_points():
    from zkvm_pairings_amd import _lib
    declared = _declared()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_engine_exposes_the_compressed_api():
    from zkvm_pairings_amd import PairingEngine, configs
    from zkvm_pairings_amd.pairings import G1Affine, G2Affine
    for name in ("fp_sqrt", "fp2_sqrt", "decompress_points", "compress_points", "decompress_points_dev", "compress_points_dev",
                 "points_check_compressed"):
        assert callable(getattr(PairingEngine, name)), name
    for cls in (G1Affine, G2Affine):
        assert callable(cls.to_compressed) and callable(cls.from_compressed)
    assert set(configs.COMPRESSED_EXPECT) == set(configs.COMPRESSED_CLASSES)


def test_host_compressor_matches_the_model():
    """configs.compress_np (the generator's host encoder, numpy only) gives the model's bytes"""
    import numpy as np
    from zkvm_pairings_amd import configs
    rng = random.Random(7)
    pts1, pts2, want1, want2 = [], [], b"", b""
    for _ in range(6):
        k = rng.randrange(1, m.R_ORDER)
        for p1, p2 in ((m.g1_mul(m.G1_GEN, k), m.g2_mul(m.G2_GEN, k)), (m.g1_neg(m.g1_mul(m.G1_GEN, k)), m.g2_neg(m.g2_mul(m.G2_GEN, k)))):
            pts1.append(configs._limbs(p1[0]).tolist() + configs._limbs(p1[1]).tolist())
            pts2.append(sum((configs._limbs(v).tolist() for v in (p2[0][0], p2[0][1], p2[1][0], p2[1][1])), []))
            want1 += cm.g1_compress(p1)
            want2 += cm.g2_compress(p2)
    assert configs.compress_np(np.array(pts1, dtype=np.uint64), 1).tobytes() == want1
    assert configs.compress_np(np.array(pts2, dtype=np.uint64), 2).tobytes() == want2
    inf = configs.compress_np(np.zeros((2, 12), dtype=np.uint64), 1, inf=[1, 1])
    assert inf.tobytes() == (bytes([0xC0]) + bytes(47)) * 2


SO = os.path.join(ROOT, "zkvm_pairings_amd", "libzkp_pairings.so")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="library not built / no llvm-readelf")
def test_compressed_kernels_use_no_scratch_and_spill_nothing():
    """the window table of the fixed-exponent power stays in registers: no private segment, no spilled register in any new kernel"""
    from test_codeobject import _kernels
    k = _kernels()
    for part in ("k_fp_sqrt", "k_fp2_sqrt", "k_g1_decompressILb1", "k_g1_decompressILb0", "k_g2_decompressILb1", "k_g2_decompressILb0",
                 "k_g1_compressILb1", "k_g1_compressILb0", "k_g2_compressILb1", "k_g2_compressILb0"):
        found = [v for n, v in k.items() if part in n]
        assert len(found) == 1, (part, found)
        v = found[0]
        assert v["spill"] == 0 and v["scratch"] == 0, (part, v)
