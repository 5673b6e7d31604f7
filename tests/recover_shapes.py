"""The shapes the recovery tests share (helper of test_recover_cpu.py, test_gpu_recover.py, test_gpu_call_order_recover.py,
test_gpu_recover_forgeries.py; not a test module).  A shape is (log2_n, log2_l): N = 2^log2_n coefficients, cells of l = 2^log2_l values, M = 2 N / l cells."""

# the model against the definition
CPU_SHAPES = [(2, 2), (3, 1), (4, 0), (4, 2), (5, 3)]

# the kernels on host threads: every M = 2^mu, mu = 1 .. 10, with l = 1 (log2_n = mu - 1) and with l = 4 (log2_n = mu + 1)
# -> (log2_n, log2_l, blobs); the third blob of a case is the one with too few cells, the largest columns carry two
KERNEL_HOST_SHAPES = [(0, 0, 3), (2, 2, 2), (2, 0, 3), (4, 2, 3), (6, 0, 2), (8, 2, 2),
                      (1, 0, 3), (3, 2, 3), (3, 0, 3), (5, 2, 3), (4, 0, 3), (6, 2, 3), (5, 0, 3), (7, 2, 3),
                      (7, 0, 3), (9, 2, 2), (8, 0, 3), (10, 2, 2), (9, 0, 2), (11, 2, 2)]

# the GPU table: (log2_n, log2_l, blobs, what it reaches); the smallest shapes that reach each path of k_rec_column and its driver
GPU_SHAPES = [
    (1, 1, 1, "one-stage column"),
    (4, 0, 3, "no cell transform"),
    (4, 2, 5, "fewer columns than a tile has slots"),
    (10, 1, 2, "the LDS limit, 512 factors in Z"),
    (12, 6, 3, "PeerDAS"),
    (11, 11, 1, "largest cell against smallest column: a cell transform of two passes, through its workspace in natural order"),
]
SMALL = (4, 2)              # the shape every pattern and every corruption case runs on
PEERDAS = (12, 6)

# one call across a slice boundary: floor(2^21 / D) blobs per slice (csrc/zkp_recover_plan.hpp), two slices, the last one of 3 blobs
SLICE_LOG2_N, SLICE_LOG2_L = 2, 1
SLICE_LEN = (1 << 21) >> (SLICE_LOG2_N + 1)
SLICE_N = SLICE_LEN + 3

# every column size: for each mu = 1 .. 10 (M = 2^mu, 2^cl = 2^(10 - mu) column slots in a tile) l = 1 (no cell transform), l = 2, l = 8
# and l = 2^(cl + 1) (two workgroups per blob, every column slot taken; at mu = 8 and mu = 10 that is the l = 8 and the l = 2 row).
# D = M l never exceeds 2^13.  -> (log2_n, log2_l, mu, cl, cols, groups): the last four are what the planner has to answer
# (test_recover_cpu.py asks it); cols: the columns of a workgroup, groups: the workgroups of a blob
EVERY_MU = [
    (0, 0, 1, 9, 1, 1), (1, 1, 1, 9, 2, 1), (3, 3, 1, 9, 8, 1), (10, 10, 1, 9, 512, 2),
    (1, 0, 2, 8, 1, 1), (2, 1, 2, 8, 2, 1), (4, 3, 2, 8, 8, 1), (10, 9, 2, 8, 256, 2),
    (2, 0, 3, 7, 1, 1), (3, 1, 3, 7, 2, 1), (5, 3, 3, 7, 8, 1), (10, 8, 3, 7, 128, 2),
    (3, 0, 4, 6, 1, 1), (4, 1, 4, 6, 2, 1), (6, 3, 4, 6, 8, 1), (10, 7, 4, 6, 64, 2),
    (4, 0, 5, 5, 1, 1), (5, 1, 5, 5, 2, 1), (7, 3, 5, 5, 8, 1), (10, 6, 5, 5, 32, 2),
    (5, 0, 6, 4, 1, 1), (6, 1, 6, 4, 2, 1), (8, 3, 6, 4, 8, 1), (10, 5, 6, 4, 16, 2),
    (6, 0, 7, 3, 1, 1), (7, 1, 7, 3, 2, 1), (9, 3, 7, 3, 8, 1), (10, 4, 7, 3, 8, 2),
    (7, 0, 8, 2, 1, 1), (8, 1, 8, 2, 2, 1), (10, 3, 8, 2, 4, 2),
    (8, 0, 9, 1, 1, 1), (9, 1, 9, 1, 2, 1), (11, 3, 9, 1, 2, 4), (10, 2, 9, 1, 2, 2),
    (9, 0, 10, 0, 1, 1), (10, 1, 10, 0, 1, 2), (12, 3, 10, 0, 1, 8),
]
EVERY_MU_KINDS = ("random-half", "one", "few")

# the single-coefficient forgeries (tests/recover_forgeries.py), all cells present: (log2_n, log2_l, the columns i0 swept or None for
# every one) - EVERY tail position t0 of each of them.  At PeerDAS shape (8 workgroups of 8 columns) the columns are sampled: the first
# and the last of the first workgroup, the first of the second, the last of the blob
FORGERY_SWEEPS = [(6, 3, None), (10, 2, None), (10, 1, None), (12, 6, (0, 7, 8, 63))]
# ... with erasures on top, a random polynomial underneath and a random factor: the GPU's shapes, which the host threads sweep too
FORGERY_ERASED = [(6, 3), (4, 2)]
# the cheapest shape on host threads whose blobs have two workgroups: M = 2, l = 1024, 512 columns each
FORGERY_HOST_GROUPS = (10, 10)

# the erasure counts at the LDS limit: the lane cuts of k_rec_vanish at degree 256 and 512 (a lane holds coefficients t, t + 256, t + 512)
# and exponents M - have of k_rec_zinv with one and with several bits set; 513 missing cells are one too many
LIMIT = (10, 1)
LIMIT_MISSING = (0, 1, 255, 256, 257, 341, 511, 512, 513)
