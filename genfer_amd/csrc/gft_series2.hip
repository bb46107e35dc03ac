// Batched bivariate series (gft_series.hpp, "rank 2"): the planner and the launches of gft_series2_mul / div / exp / log / compose /
// corr / compose_adj, for F64 and (the first five) for Interval<F64> (the element width w of the entry point: SeriesPlanes).  The
// kernels are in gft_series2_kernels.hpp; gfx950 only.  pow is series_pow (gft_series.hip) over this file's SERIES_MUL launch.
//
// One form: one workgroup per item for the whole operation.
//   lanes    one wave while the item has at most 64 coefficients, else up to 256 in whole waves: mul counts its output PAIRS (a
//            thread owns two outputs), div / exp / log the coefficients n0 * n1 (the widest pass forms up to that many row sums).
//   LDS      mul: x and y compact, at most 64 KB.  div / exp / log: the resident operand (y, x) and the result, at most 64 KB,
//            and behind them the scratch of the row sums: as many rows of n1 doubles as the longest j range has terms, capped by
//            what the 80 KB request of the univariate form A leaves (two workgroups of 80 KB share a CU's 160 KB).  An item at the
//            4096 limit keeps 16 KB of scratch, which is one row of the longest row that has a second one (n0 = 2, n1 = 2048).
//            Where the runtime grants only 64 KB an item whose arrays and one scratch row do not fit is refused by name.
//            compose: two result arrays of n0 * n1 doubles taking turns, at most 64 KB, and g compact behind them where the three
//            fit the grant of that 80 KB request; otherwise g stays in global memory, so every admissible shape runs on 64 KB.
// Intervals (w == 2): an LDS element is 16 bytes, so every footprint above is reached at half the coefficients -- the limit is 2048
// (SERIES2_MAX_ELEMS_IV), two resident arrays are the same 64 KB, and the scratch rows, compose's GLDS decision and the refusal
// scale with the width.  The LDS requests and what the runtime answered are kept per element type.
// compose's lanes count mul's output pairs of the full shape, in whole waves up to 512 (measured: S2_COMPOSE_LANES).
// The transposed operations (F64 only; x is the LONG side, g resp. gh, and the result the short one): corr has mul's plan with the
// lanes counted over the output pairs of the result; compose_adj has compose's plan on gh's shape -- two arrays of nx0 * nx1 doubles
// and g beside them where the grant holds all three -- and its own measured lane count (S2_ADJ_LANES).
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

// what the runtime grants the three recurrence kernels and compose / compose_adj with g resident, asked once
size_t s2_budget(int w) {
    static size_t answers[2] = {0, 0};
    size_t& granted = answers[w == 2];
    if (granted) return granted;
    const void* kf[] = {(const void*)k_series2_rec<SERIES_DIV>, (const void*)k_series2_rec<SERIES_EXP>, (const void*)k_series2_rec<SERIES_LOG>,
                        (const void*)k_series2_compose<true>, (const void*)k_series2_compose_adj<EF64, true>};
    const void* ki[] = {(const void*)k_series2i_rec<EIv, SERIES_DIV>, (const void*)k_series2i_rec<EIv, SERIES_EXP>,
                        (const void*)k_series2i_rec<EIv, SERIES_LOG>, (const void*)k_series2i_compose<EIv, true>};
    granted = w == 2 ? grant_dynamic_lds(ki, sizeof(ki) / sizeof(*ki), S2_BUDGET, S2_BUDGET_PLAIN)
                     : grant_dynamic_lds(kf, sizeof(kf) / sizeof(*kf), S2_BUDGET, S2_BUDGET_PLAIN);
    return granted;
}

// compose: two waves a SIMD on the large items.  Measured on (256, 32, 32) / (256, 64, 64) / (64, 32, 128) items: 256 lanes 1.93 / 67.3 /
// 27.4 ms, 512 lanes 1.23 / 59.0 / 22.0 ms, 1024 lanes 1.23 / 59.9 / 22.5 ms (profiles/r12/series2_compose_lanes.json).
constexpr unsigned S2_COMPOSE_LANES = 512;
// compose_adj, as compose: two waves a SIMD.  Measured on 256 items of f = g = n = (32, 32), var 0 / var 1, two builds alternating in
// one run: 256 lanes 1.87 / 1.86 ms, 512 lanes 1.25 / 1.24 ms (profiles/r14/series2_adj_lanes.json).
constexpr unsigned S2_ADJ_LANES = 512;

}  // namespace

Series2Plan series2_plan(int op, const Series2Dims& d, int w) {
    Series2Plan p;
    const size_t elem = (size_t)w * sizeof(double);  // of an LDS element
    const unsigned N = d.n0 * d.n1;
    if (op == SERIES_MUL || op == SERIES_CORR) {  // (corr: N counts the result m, and g and y <= g are 64 KB at most as well)
        p.threads = series_threads((N + 1) / 2);
        p.srows = 0;
        p.lds = ((size_t)d.nx0 * d.nx1 + (size_t)d.ny0 * d.ny1) * elem;
        return p;
    }
    if (op == SERIES_COMPOSE || op == SERIES_COMPOSE_ADJ) {
        const bool adj = op == SERIES_COMPOSE_ADJ;
        const unsigned A = adj ? d.nx0 * d.nx1 : N;  // of an array taking turns: the composition's shape (compose_adj: gh's)
        const size_t rows = (size_t)2 * A * elem, all = rows + (size_t)d.ny0 * d.ny1 * elem;
        p.threads = series_threads((A + 1) / 2, adj ? S2_ADJ_LANES : S2_COMPOSE_LANES);
        p.srows = 0;
        p.glds = all <= S2_BUDGET_PLAIN || all <= s2_budget(w);
        p.lds = p.glds ? all : rows;
        return p;
    }
    const unsigned a0 = op == SERIES_DIV ? d.ny0 : d.nx0, a1 = op == SERIES_DIV ? d.ny1 : d.nx1;
    const size_t resident = ((size_t)a0 * a1 + N) * elem, row = (size_t)d.n1 * elem;
    unsigned terms = std::min(d.n0, a0) - 1;  // of the longest j range (log's starts at 1: one term fewer while k < nx0)
    if (op == SERIES_LOG && d.n0 <= a0) terms = d.n0 >= 2 ? d.n0 - 2 : 0;
    p.threads = series_threads(N);
    p.srows = 0;
    if (terms) {
        const size_t budget = s2_budget(w);
        if (resident + row > budget)
            throw std::runtime_error("series2: an item of " + std::to_string(d.n0) + " x " + std::to_string(d.n1) + " coefficients" + (w == 2 ? " of two bounds" : "") + " needs " +
                                     std::to_string(resident + row) + " bytes of LDS (two resident arrays and one scratch row), but the runtime grants " +
                                     std::to_string(budget) + " bytes per workgroup");
        p.srows = (unsigned)std::min<size_t>(terms, (budget - resident) / row);
    }
    p.lds = resident + p.srows * row;
    return p;
}

void series2_launch(hipStream_t st, int op, const Series2Plan& p, const double* x, const double* y, double* res, const Series2Dims& d,
                    const SeriesBatch& g, int var, const SeriesPlanes& pl) {
    if (g.items == 0) return;
    const dim3 grid(g.items), block(p.threads);
    if (pl.w == 2) {
        switch (op) {
            case SERIES_MUL: GFT_LAUNCH(k_series2i_mul<EIv>, grid, block, p.lds, st, x, y, res, d, g, pl); break;
            case SERIES_DIV: GFT_LAUNCH((k_series2i_rec<EIv, SERIES_DIV>), grid, block, p.lds, st, x, y, res, d, p.srows, g, pl); break;
            case SERIES_EXP: GFT_LAUNCH((k_series2i_rec<EIv, SERIES_EXP>), grid, block, p.lds, st, x, y, res, d, p.srows, g, pl); break;
            case SERIES_LOG: GFT_LAUNCH((k_series2i_rec<EIv, SERIES_LOG>), grid, block, p.lds, st, x, y, res, d, p.srows, g, pl); break;
            case SERIES_COMPOSE:
                if (p.glds) GFT_LAUNCH((k_series2i_compose<EIv, true>), grid, block, p.lds, st, x, y, res, d, var, g, pl);
                else GFT_LAUNCH((k_series2i_compose<EIv, false>), grid, block, p.lds, st, x, y, res, d, var, g, pl);
                break;
            default: throw std::runtime_error("series2: no such operation at rank 2");
        }
        return;
    }
    switch (op) {
        case SERIES_MUL: GFT_LAUNCH(k_series2_mul, grid, block, p.lds, st, x, y, res, d, g); break;
        case SERIES_CORR: GFT_LAUNCH(k_series2_corr<EF64>, grid, block, p.lds, st, x, y, res, d, g); break;
        case SERIES_COMPOSE_ADJ:
            if (p.glds) GFT_LAUNCH((k_series2_compose_adj<EF64, true>), grid, block, p.lds, st, x, y, res, d, var, g);
            else GFT_LAUNCH((k_series2_compose_adj<EF64, false>), grid, block, p.lds, st, x, y, res, d, var, g);
            break;
        case SERIES_DIV: GFT_LAUNCH(k_series2_rec<SERIES_DIV>, grid, block, p.lds, st, x, y, res, d, p.srows, g); break;
        case SERIES_EXP: GFT_LAUNCH(k_series2_rec<SERIES_EXP>, grid, block, p.lds, st, x, y, res, d, p.srows, g); break;
        case SERIES_LOG: GFT_LAUNCH(k_series2_rec<SERIES_LOG>, grid, block, p.lds, st, x, y, res, d, p.srows, g); break;
        case SERIES_COMPOSE:
            if (p.glds) GFT_LAUNCH(k_series2_compose<true>, grid, block, p.lds, st, x, y, res, d, var, g);
            else GFT_LAUNCH(k_series2_compose<false>, grid, block, p.lds, st, x, y, res, d, var, g);
            break;
        default: throw std::runtime_error("series2: no such operation at rank 2");
    }
}

}  // namespace gft
