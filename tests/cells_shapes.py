"""The shapes at which the cell proofs' planner (csrc/zkp_cells_plan.hpp: group_log2) takes each of its group sizes g, shared by
test_cells_cpu.py - which asks the planner itself, through tests/cells_plan_check.cpp, and asserts that every g is reached - and by
test_gpu_cells.py, which runs them.  (n, log2_n, log2_l, log2_ext, g expected).  2 n N lanes at g = 1: g = 1 up to 2^16 of them, then the
smallest of 2, 4 that brings them back to 2^16, never above l.  Not a test module."""

G_SHAPES = [
    (512, 6, 3, 1, 1),       # 2^16 lanes exactly: the last shape of g = 1
    (513, 6, 3, 1, 2),       # one polynomial more
    (1025, 6, 3, 1, 4),      # above 2^17: g = 4, two partials per slot
    (1025, 6, 1, 0, 2),      # l = 2 caps g: the chain writes the record itself, no partials
]
G_VALUES = (1, 2, 4)

# The shapes at which test_gpu_cells.py makes the additions of k_cell_mac and k_cell_sum meet their exceptional cases, and
# test_cells_cpu.py shows on the model (cells_model.addition_cases) that they do: (n, log2_n, log2_l, log2_ext, g).  Equal bases AND equal
# scalars are needed: a setup with tau = 1 makes the l setup vectors equal, tau = -1 (r - 1) makes them alternate in sign, and a
# polynomial whose coefficients are all equal makes the l scalars of a slot equal.  With g = 1 the equal (opposite) partials meet in the
# sum; with g > 1 the equal (opposite) bases meet inside a lane, at the first bit their scalars share.
EXCEPTIONAL_SHAPES = [
    (6, 6, 2, 1, 1),         # four partials per slot
    (513, 6, 3, 1, 2),       # two bases per lane, four partials per slot
    (1025, 6, 3, 1, 4),      # four bases per lane, two partials per slot
]
