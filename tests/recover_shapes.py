"""The shapes the recovery tests share (helper of test_recover_cpu.py, test_gpu_recover.py, test_gpu_call_order_recover.py; not a test
module).  A shape is (log2_n, log2_l): N = 2^log2_n coefficients, cells of l = 2^log2_l values, M = 2 N / l cells."""

# the model against the definition
CPU_SHAPES = [(2, 2), (3, 1), (4, 0), (4, 2), (5, 3)]

# the kernels on host threads: M = 2, 8 and 128 with l = 1 and l = 4 -> (log2_n, log2_l, blobs)
KERNEL_HOST_SHAPES = [(0, 0, 3), (2, 2, 2), (2, 0, 3), (4, 2, 3), (6, 0, 2), (8, 2, 2)]

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
