// cell_verify_plan_check.cpp -- what the planners of zkp_kzg_cell_verify_batch answer for the shapes of tests/test_gpu_cell_verify.py: the
// fold's grid (zkp_groth16_plan.hpp, fold_plan(n, l)), the inverse transform's passes and workspace (zkp_poly_plan.hpp) and the verifier's
// layout (zkp_cells_plan.hpp, verify_layout) under every flag combination.  A stand-alone program built with g++ -fsanitize=address,undefined
// (tests/test_cell_verify_cpu.py compiles and runs it as a child process).  Reads "log2_d log2_l n" lines from stdin and prints, per line,
//   log2_d log2_l n  tw rows tiles parts last_rows  passes_natural ws_natural passes_bitrev ws_bitrev  layouts
// last_rows: the rows the last part of the fold holds when every part takes one run of rows (parts = ceil(n / rows)), else 0; layouts: the
// number of (order, flags) layouts whose offsets were found increasing, 256-aligned and wide enough for what the driver writes.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../zkvm_pairings_amd/csrc/zkp_cells_plan.hpp"
#include "../zkvm_pairings_amd/csrc/zkp_groth16_plan.hpp"
#include "../zkvm_pairings_amd/csrc/zkp_poly_plan.hpp"

namespace cl = zkp::cells;
namespace g16 = zkp::g16;
namespace poly = zkp::poly;

static bool layout_ok(size_t n, unsigned log2_l, int flags, size_t ntt_bytes, size_t part_bytes) {
    const cl::VerifyLayout L = cl::verify_layout(n, log2_l, flags, ntt_bytes, part_bytes);
    const size_t l = (size_t)1 << log2_l, m = 2 * n + l;
    const size_t n_status = ((flags & cl::VERIFY_POINTS_CHECKED) ? 0 : 2 * n) + ((flags & cl::VERIFY_VK_CHECKED) ? 0 : l + 2);
    if (L.n_status != n_status) return false;
    // the regions in the order of the layout, with the bytes the driver writes into each
    const size_t at[] = {L.flag, L.st, L.coef, L.ntt, L.ms, L.mp, L.minf, L.part, L.a, L.mg1, L.minf1, L.mg2, L.ml, L.total};
    const size_t bytes[] = {8, n_status, n * l * 32, ntt_bytes, 2 * m * 32, m * 96, m, part_bytes, l * 32, 2 * 96, 2, 2 * 192, 2 * 576};
    for (int i = 0; i < 13; i++)
        if (at[i] % 256 || at[i] + bytes[i] > at[i + 1] || (bytes[i] && at[i] >= at[i + 1])) return false;
    return L.flag == 0 && L.total % 256 == 0;
}

int main() {
    unsigned log2_d, log2_l;
    unsigned long n;
    int lines = 0;
    while (scanf("%u %u %lu", &log2_d, &log2_l, &n) == 3) {
        int layouts = 0;
        for (int order : {0, (int)poly::NTT_BITREV})
            for (int checked : {0, 4, 8, 12}) {
                if (cl::verify_args_bad(n, log2_d, log2_l, order | checked) || !n) {
                    fprintf(stderr, "the ABI refuses %u %u %lu under flags %d\n", log2_d, log2_l, n, order | checked);
                    return 1;
                }
            }
        const size_t l = (size_t)1 << log2_l;
        if (g16::fold_args_bad(n, l)) return 1;
        const g16::FoldPlan fp = g16::fold_plan(n, l);
        const size_t need = (n + fp.rows - 1) / fp.rows;
        const size_t last = fp.parts == need ? n - (size_t)(fp.parts - 1) * fp.rows : 0;
        size_t ws[2];
        int passes[2];
        for (int b = 0; b < 2; b++) {
            const int nflags = poly::NTT_INVERSE | (b ? poly::NTT_BITREV : 0);
            if (poly::ntt_args_bad(n, log2_l, nflags)) return 1;
            const poly::Plan P = poly::make_plan(n, log2_l, nflags);
            if (!P.ok || P.workspace != (poly::ntt_workspace_bytes(n, log2_l, nflags) > 0)) return 1;
            ws[b] = poly::ntt_workspace_bytes(n, log2_l, nflags);
            passes[b] = P.n_pass;
            for (int checked : {0, 4, 8, 12}) layouts += layout_ok(n, log2_l, (b ? poly::NTT_BITREV : 0) | checked, ws[b], fp.part_bytes);
        }
        printf("%u %u %lu  %u %u %u %u %zu  %d %zu %d %zu  %d\n", log2_d, log2_l, n, fp.tw, fp.rows, fp.tiles, fp.parts, last, passes[0], ws[0], passes[1], ws[1],
               layouts);
        lines++;
    }
    printf("cell verify plan_check ok: %d shapes\n", lines);
    return 0;
}
