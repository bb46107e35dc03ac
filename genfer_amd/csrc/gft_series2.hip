// Batched bivariate series (gft_series.hpp, "rank 2"): the planner and the launches of gft_series2_mul / div / exp / log.  The
// kernels are in gft_series2_kernels.hpp; gfx950 only, f64 only.
//
// One form: one workgroup per item for the whole operation.
//   lanes    one wave while the item has at most 64 coefficients, else up to 256 in whole waves: mul counts its output PAIRS (a
//            thread owns two outputs), div / exp / log the coefficients n0 * n1 (the widest pass forms up to that many row sums).
//   LDS      mul: x and y compact, at most 64 KB.  div / exp / log: the resident operand (y, x) and the result, at most 64 KB,
//            and behind them the scratch of the row sums: as many rows of n1 doubles as the longest j range has terms, capped by
//            what the 80 KB request of the univariate form A leaves (two workgroups of 80 KB share a CU's 160 KB).  An item at the
//            4096 limit keeps 16 KB of scratch, which is one row of the longest row that has a second one (n0 = 2, n1 = 2048).
//            Where the runtime grants only 64 KB an item whose arrays and one scratch row do not fit is refused by name.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "gft_launch.hpp"
#include "gft_series.hpp"
#include "gft_series2_kernels.hpp"

namespace gft {

namespace {

constexpr size_t S2_BUDGET = 80 * 1024, S2_BUDGET_PLAIN = 64 * 1024;

// what the runtime grants the three recurrence kernels, asked once
size_t s2_budget() {
    static size_t granted = 0;
    if (granted) return granted;
    const void* ks[] = {(const void*)k_series2_rec<SERIES_DIV>, (const void*)k_series2_rec<SERIES_EXP>, (const void*)k_series2_rec<SERIES_LOG>};
    granted = S2_BUDGET;
    for (const void* k : ks)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S2_BUDGET) != hipSuccess) {
            (void)hipGetLastError();  // no stale error for the caller's next HIP call
            granted = S2_BUDGET_PLAIN;
            break;
        }
    return granted;
}

unsigned s2_threads(unsigned work) { return work <= 64 ? 64u : std::min(256u, (work + 63) / 64 * 64); }

}  // namespace

Series2Plan series2_plan(int op, const Series2Dims& d) {
    Series2Plan p;
    const unsigned N = d.n0 * d.n1;
    if (op == SERIES_MUL) {
        p.threads = s2_threads((N + 1) / 2);
        p.srows = 0;
        p.lds = ((size_t)d.nx0 * d.nx1 + (size_t)d.ny0 * d.ny1) * sizeof(double);
        return p;
    }
    const unsigned a0 = op == SERIES_DIV ? d.ny0 : d.nx0, a1 = op == SERIES_DIV ? d.ny1 : d.nx1;
    const size_t resident = ((size_t)a0 * a1 + N) * sizeof(double), row = (size_t)d.n1 * sizeof(double);
    unsigned terms = std::min(d.n0, a0) - 1;  // of the longest j range (log's starts at 1: one term fewer while k < nx0)
    if (op == SERIES_LOG && d.n0 <= a0) terms = d.n0 >= 2 ? d.n0 - 2 : 0;
    p.threads = s2_threads(N);
    p.srows = 0;
    if (terms) {
        const size_t budget = s2_budget();
        if (resident + row > budget)
            throw std::runtime_error("series2: an item of " + std::to_string(d.n0) + " x " + std::to_string(d.n1) + " coefficients needs " +
                                     std::to_string(resident + row) + " bytes of LDS (two resident arrays and one scratch row), but the runtime grants " +
                                     std::to_string(budget) + " bytes per workgroup");
        p.srows = (unsigned)std::min<size_t>(terms, (budget - resident) / row);
    }
    p.lds = resident + p.srows * row;
    return p;
}

void series2_launch(hipStream_t st, int op, const Series2Plan& p, const double* x, const double* y, double* res, const Series2Dims& d,
                    const SeriesBatch& g) {
    if (g.items == 0) return;
    const dim3 grid(g.items), block(p.threads);
    switch (op) {
        case SERIES_MUL: GFT_LAUNCH(k_series2_mul, grid, block, p.lds, st, x, y, res, d, g); break;
        case SERIES_DIV: GFT_LAUNCH(k_series2_rec<SERIES_DIV>, grid, block, p.lds, st, x, y, res, d, p.srows, g); break;
        case SERIES_EXP: GFT_LAUNCH(k_series2_rec<SERIES_EXP>, grid, block, p.lds, st, x, y, res, d, p.srows, g); break;
        case SERIES_LOG: GFT_LAUNCH(k_series2_rec<SERIES_LOG>, grid, block, p.lds, st, x, y, res, d, p.srows, g); break;
        default: throw std::runtime_error("series2: no such operation at rank 2");
    }
}

}  // namespace gft
