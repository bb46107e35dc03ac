// Batched trivariate series (gft_series.hpp, "rank 3"): the planner and the launches of gft_series3_mul / div / exp / log, F64 only.
// The kernels are in gft_series3_kernels.hpp; gfx950 only.  Nothing about these choices has been measured beyond the table of
// they are rank 2's (gft_series2.hip), counted the same way.
//
// One form: one workgroup per item for the whole operation, on the permuted item of Series3Dims (the unit axes of S in front).
//   lanes    one wave while the item has at most 64 units of parallel work, else up to 256 in whole waves: mul counts its output
//            PAIRS, div / exp / log the coefficients of S.
//   LDS      mul: x and y compact, at most 64 KB.  div / exp / log: the resident operand (y, x) and the result, at most 64 KB, and
//            behind them the scratch of the row sums, out of the same 80 KB request as rank 2.  A chunk of terms is `tc` slabs of
//            n1 * n2 doubles; an item with a second slab has slabs of at most 2048 coefficients, so one always fits, and the
//            rank-2 step of a slab (one row of accumulators, one of row sums) fits inside it.  An item of ONE slab is the rank-2
//            item and is sized as series2_plan sizes it: rows of n2 doubles, one at least.  Where the runtime grants only 64 KB an
//            item whose arrays and smallest scratch do not fit is refused by name.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "gft_launch.hpp"
#include "gft_series.hpp"
#include "gft_series3_kernels.hpp"

namespace gft {

namespace {

constexpr size_t S3_BUDGET = 80 * 1024, S3_BUDGET_PLAIN = 64 * 1024;

// what the runtime grants the three recurrence kernels, asked once
size_t s3_budget() {
    static size_t granted = 0;
    if (granted) return granted;
    const void* ks[] = {(const void*)k_series3_rec<SERIES_DIV>, (const void*)k_series3_rec<SERIES_EXP>, (const void*)k_series3_rec<SERIES_LOG>};
    granted = S3_BUDGET;
    for (const void* k : ks)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S3_BUDGET) != hipSuccess) {
            (void)hipGetLastError();  // no stale error for the caller's next HIP call
            granted = S3_BUDGET_PLAIN;
            break;
        }
    return granted;
}

unsigned s3_threads(unsigned work) { return work <= 64 ? 64u : std::min(256u, (work + 63) / 64 * 64); }

}  // namespace

Series3Plan series3_plan(int op, const Series3Dims& d) {
    Series3Plan p;
    const size_t elem = sizeof(double);
    const unsigned n12 = d.n[1] * d.n[2], N = d.n[0] * n12;
    if (op == SERIES_MUL) {
        p.threads = s3_threads((N + 1) / 2);
        p.lds = ((size_t)d.nx[0] * d.nx[1] * d.nx[2] + (size_t)d.ny[0] * d.ny[1] * d.ny[2]) * elem;
        return p;
    }
    const unsigned* a = op == SERIES_DIV ? d.ny : d.nx;
    const size_t resident = (size_t)a[0] * a[1] * a[2] + N;                    // elements
    const unsigned terms0 = std::min(d.n[0], a[0]) - 1, J1 = std::min(d.n[1], a[1]);  // of the longest j0 range; places of j1
    const unsigned terms2 = J1 - 1;                                            // of the longest j range of a rank-2 row
    // the smallest scratch and the one that takes every term at once
    size_t need, want;
    if (d.n[0] == 1) need = terms2 ? d.n[2] : 0, want = (size_t)terms2 * d.n[2];
    else need = n12, want = std::max<size_t>((size_t)terms0 * J1, 1) * n12;
    p.threads = s3_threads(N);
    if (need) {
        const size_t budget = s3_budget();
        if ((resident + need) * elem > budget)
            throw std::runtime_error("series3: an item of " + std::to_string(d.n[0]) + " x " + std::to_string(d.n[1]) + " x " + std::to_string(d.n[2]) +
                                     " coefficients needs " + std::to_string((resident + need) * elem) +
                                     " bytes of LDS (two resident arrays and the smallest scratch), but the runtime grants " + std::to_string(budget) +
                                     " bytes per workgroup");
        p.selems = (unsigned)std::min(want, budget / elem - resident);
    }
    p.tc = d.n[0] == 1 ? 0 : (unsigned)std::min<size_t>((size_t)terms0 * J1, p.selems / n12);
    p.lds = (resident + p.selems) * elem;
    return p;
}

void series3_launch(hipStream_t st, int op, const Series3Plan& p, const double* x, const double* y, double* res, const Series3Dims& d,
                    const SeriesBatch& g) {
    if (g.items == 0) return;
    const dim3 grid(g.items), block(p.threads);
    switch (op) {
        case SERIES_MUL: GFT_LAUNCH(k_series3_mul, grid, block, p.lds, st, x, y, res, d, g); break;
        case SERIES_DIV: GFT_LAUNCH(k_series3_rec<SERIES_DIV>, grid, block, p.lds, st, x, y, res, d, p.tc, p.selems, g); break;
        case SERIES_EXP: GFT_LAUNCH(k_series3_rec<SERIES_EXP>, grid, block, p.lds, st, x, y, res, d, p.tc, p.selems, g); break;
        case SERIES_LOG: GFT_LAUNCH(k_series3_rec<SERIES_LOG>, grid, block, p.lds, st, x, y, res, d, p.tc, p.selems, g); break;
        default: throw std::runtime_error("series3: no such operation at rank 3");
    }
}

}  // namespace gft
