"""The shapes the bucket-MSM GPU tests run (tests/test_gpu_msm_shapes.py), each with the plan it is meant to reach in
zkvm_pairings_amd/csrc/zkp_msm_plan.hpp: window width c, passes, bucket-reduction split and chunk, accumulation levels.
tests/test_msm_cpu.py compiles make_plan on the CPU and asserts that every row gets exactly these fields and that the rows
together cover every c for G1 and G2, both ends of every c range, multi-pass calls with a partial last pass and the largest
admitted call - so a change to choose_c or to the pass split that moves the GPU tests off these shapes fails on the CPU."""
from collections import namedtuple

MAX_TERMS = 1 << 24

# segs: segments per pass; groups: which of G1 (1) and G2 (2) run the row on the GPU
Shape = namedtuple("Shape", "m n_msm shared c passes split chunk levels segs groups")

# every window width at both ends of its range of m (G1); the low ends run for G2 too.  n_msm > 1 where it moves the reduction to
# chunk > 1 at a smaller split.
WIDTHS = [
    Shape(1, 64, False, 2, 1, 2, 1, 4, 64, (1, 2)),
    Shape(6, 16, False, 2, 1, 2, 1, 4, 16, (1,)),
    Shape(7, 128, False, 3, 1, 2, 2, 4, 128, (1, 2)),
    Shape(25, 4, True, 3, 1, 4, 1, 4, 4, (1,)),
    Shape(26, 64, False, 4, 1, 4, 2, 4, 64, (1, 2)),
    Shape(72, 2, False, 4, 1, 8, 1, 4, 2, (1,)),
    Shape(73, 48, True, 5, 1, 8, 2, 5, 48, (1, 2)),
    Shape(181, 2, False, 5, 1, 16, 1, 4, 2, (1,)),
    Shape(182, 32, False, 6, 1, 16, 2, 5, 32, (1, 2)),
    Shape(496, 1, False, 6, 1, 32, 1, 4, 1, (1,)),
    Shape(497, 16, True, 7, 1, 32, 2, 5, 16, (1, 2)),
    Shape(1392, 1, False, 7, 1, 64, 1, 4, 1, (1,)),
    Shape(1393, 16, False, 8, 1, 32, 4, 5, 16, (1, 2)),
    Shape(2400, 1, False, 8, 1, 128, 1, 4, 1, (1,)),
    Shape(2401, 12, True, 9, 1, 64, 4, 5, 12, (1, 2)),
    Shape(5888, 1, False, 9, 1, 256, 1, 5, 1, (1,)),
    Shape(5889, 6, False, 10, 1, 128, 4, 5, 6, (1, 2)),
    Shape(16896, 1, False, 10, 1, 512, 1, 5, 1, (1,)),
    Shape(16897, 2, True, 11, 1, 512, 2, 5, 2, (1, 2)),
    Shape(30720, 1, False, 11, 1, 1024, 1, 5, 1, (1,)),
    Shape(30721, 4, False, 12, 1, 256, 8, 6, 4, (1, 2)),
    Shape(55296, 1, False, 12, 1, 1024, 2, 5, 1, (1,)),
    Shape(55297, 1, False, 13, 1, 1024, 4, 5, 1, (1, 2)),
    Shape(221184, 1, False, 13, 1, 1024, 4, 6, 1, (1,)),
    Shape(221185, 1, False, 14, 1, 1024, 8, 6, 1, (1, 2)),
    Shape(417792, 1, False, 14, 1, 1024, 8, 6, 1, (1,)),
    Shape(417793, 1, False, 15, 1, 1024, 16, 6, 1, (1, 2)),
    Shape(786432, 1, False, 15, 1, 1024, 16, 6, 1, (1,)),
    Shape(786433, 1, False, 16, 1, 1024, 32, 6, 1, (1, 2)),
    Shape(MAX_TERMS, 1, False, 16, 1, 1024, 32, 7, 1, (1,)),      # the largest admitted call
]

# three passes of 65027 segments, the last one partial (9946 segments); split 1, chunk 2
PASSES = [
    Shape(1, 140000, False, 2, 3, 1, 2, 6, 65027, (1,)),
    Shape(2, 140000, False, 2, 3, 1, 2, 6, 65027, (1, 2)),
    Shape(3, 140000, True, 2, 3, 1, 2, 6, 65027, (1,)),
]

# msm_profile against the plain call: one multi-pass and one one-pass shape
PROFILE = [PASSES[1], WIDTHS[12]]

ALL = WIDTHS + PASSES
