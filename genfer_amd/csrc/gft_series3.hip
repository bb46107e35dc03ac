// Batched trivariate series (gft_series.hpp, "rank 3"): the planner and the launches of gft_series3_mul / div / exp / log / compose,
// for F64 and for Interval<F64> (the element width w of the entry point: SeriesPlanes).  The kernels are in gft_series3_kernels.hpp;
// gfx950 only.  pow is series_pow (gft_series.hip) over this file's SERIES_MUL launch.  The choices for mul / div / exp / log have not been measured beyond the tables of
// they are rank 2's (gft_series2.hip), counted the same way; compose's lane count has its own sweep (DESIGN
// 3.23).
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
//            compose: two result arrays of n0 * n1 * n2 doubles taking turns, at most 64 KB, and g compact behind them where the
//            three fit 64 KB or the grant of that 80 KB request; otherwise g stays in global memory, so every admissible shape runs
//            on 64 KB.
// Intervals (w == 2): an LDS element is 16 bytes, so every footprint above is reached at half the coefficients -- the limit is 2048
// (SERIES3_MAX_ELEMS_IV), two resident arrays are the same 64 KB, an item with a second slab has slabs of at most 1024 elements
// (16 KB: one chunk fits), and the scratch, compose's GLDS decision and the refusal scale with the width.  The LDS requests and what
// the runtime answered are kept per element type.
// compose's lanes count mul's output pairs of the full shape, in whole waves up to S3_COMPOSE_LANES.
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

// what the runtime grants the three recurrence kernels and compose with g resident, asked once
size_t s3_budget(int w) {
    static size_t answers[2] = {0, 0};
    size_t& granted = answers[w == 2];
    if (granted) return granted;
    const void* kf[] = {(const void*)k_series3_rec<SERIES_DIV>, (const void*)k_series3_rec<SERIES_EXP>, (const void*)k_series3_rec<SERIES_LOG>,
                        (const void*)k_series3_compose<true>};
    const void* ki[] = {(const void*)k_series3i_rec<EIv, SERIES_DIV>, (const void*)k_series3i_rec<EIv, SERIES_EXP>,
                        (const void*)k_series3i_rec<EIv, SERIES_LOG>, (const void*)k_series3i_compose<EIv, true>};
    granted = grant_dynamic_lds(w == 2 ? ki : kf, 4, S3_BUDGET, S3_BUDGET_PLAIN);
    return granted;
}

// compose: rank 2's rule (S2_COMPOSE_LANES), whole waves over the output pairs up to two waves a SIMD; the sweep of 256 / 512 / 1024
// lanes at rank 3 is in DESIGN 3.23 (profiles/r20/series3_compose_lanes.json).
constexpr unsigned S3_COMPOSE_LANES = 512;

}  // namespace

Series3Plan series3_plan(int op, const Series3Dims& d, int w) {
    Series3Plan p;
    const size_t elem = (size_t)w * sizeof(double);  // of an LDS element
    const unsigned n12 = d.n[1] * d.n[2], N = d.n[0] * n12;
    if (op == SERIES_MUL) {
        p.threads = series_threads((N + 1) / 2);
        p.lds = ((size_t)d.nx[0] * d.nx[1] * d.nx[2] + (size_t)d.ny[0] * d.ny[1] * d.ny[2]) * elem;
        return p;
    }
    // the device-free arithmetic is series3_sizes (gft_series_args.hpp); the grant is asked only where an item needs scratch
    Series3Sizes z = series3_sizes(op, d, w, S3_BUDGET);
    p.threads = series_threads(N);
    if (z.need) {
        const size_t budget = s3_budget(w);
        if (budget != S3_BUDGET) z = series3_sizes(op, d, w, budget);
        if (!z.fits)
            throw std::runtime_error("series3: an item of " + std::to_string(d.n[0]) + " x " + std::to_string(d.n[1]) + " x " + std::to_string(d.n[2]) +
                                     " coefficients" + (w == 2 ? " of two bounds" : "") + " needs " + std::to_string((z.resident + z.need) * elem) +
                                     " bytes of LDS (two resident arrays and the smallest scratch), but the runtime grants " + std::to_string(budget) +
                                     " bytes per workgroup");
    }
    p.selems = z.selems;
    p.tc = z.tc;
    p.lds = (z.resident + z.selems) * elem;
    return p;
}

Series3Plan series3_compose_plan(const Series3Compose& c, int w) {
    Series3Plan p;
    const size_t N = (size_t)c.full[0] * c.full[1] * c.full[2], elem = (size_t)w * sizeof(double);
    const size_t arrays = 2 * N * elem, all = arrays + (size_t)c.ng[0] * c.ng[1] * c.ng[2] * elem;
    p.threads = series_threads((unsigned)((N + 1) / 2), S3_COMPOSE_LANES);
    p.glds = all <= S3_BUDGET_PLAIN || all <= s3_budget(w);
    p.lds = p.glds ? all : arrays;
    return p;
}

void series3_compose_launch(hipStream_t st, const Series3Plan& p, const double* f, const double* g, double* res, const Series3Compose& c,
                            const SeriesBatch& b, const SeriesPlanes& pl) {
    if (b.items == 0) return;
    const dim3 grid(b.items), block(p.threads);
    if (pl.w == 2) {
        if (p.glds) GFT_LAUNCH((k_series3i_compose<EIv, true>), grid, block, p.lds, st, f, g, res, c, b, pl);
        else GFT_LAUNCH((k_series3i_compose<EIv, false>), grid, block, p.lds, st, f, g, res, c, b, pl);
        return;
    }
    if (p.glds) GFT_LAUNCH(k_series3_compose<true>, grid, block, p.lds, st, f, g, res, c, b);
    else GFT_LAUNCH(k_series3_compose<false>, grid, block, p.lds, st, f, g, res, c, b);
}

void series3_launch(hipStream_t st, int op, const Series3Plan& p, const double* x, const double* y, double* res, const Series3Dims& d,
                    const SeriesBatch& g, const SeriesPlanes& pl) {
    if (g.items == 0) return;
    const dim3 grid(g.items), block(p.threads);
    if (pl.w == 2) {
        switch (op) {
            case SERIES_MUL: GFT_LAUNCH(k_series3i_mul<EIv>, grid, block, p.lds, st, x, y, res, d, g, pl); break;
            case SERIES_DIV: GFT_LAUNCH((k_series3i_rec<EIv, SERIES_DIV>), grid, block, p.lds, st, x, y, res, d, p.tc, p.selems, g, pl); break;
            case SERIES_EXP: GFT_LAUNCH((k_series3i_rec<EIv, SERIES_EXP>), grid, block, p.lds, st, x, y, res, d, p.tc, p.selems, g, pl); break;
            case SERIES_LOG: GFT_LAUNCH((k_series3i_rec<EIv, SERIES_LOG>), grid, block, p.lds, st, x, y, res, d, p.tc, p.selems, g, pl); break;
            default: throw std::runtime_error("series3: no such operation at rank 3");
        }
        return;
    }
    switch (op) {
        case SERIES_MUL: GFT_LAUNCH(k_series3_mul, grid, block, p.lds, st, x, y, res, d, g); break;
        case SERIES_DIV: GFT_LAUNCH(k_series3_rec<SERIES_DIV>, grid, block, p.lds, st, x, y, res, d, p.tc, p.selems, g); break;
        case SERIES_EXP: GFT_LAUNCH(k_series3_rec<SERIES_EXP>, grid, block, p.lds, st, x, y, res, d, p.tc, p.selems, g); break;
        case SERIES_LOG: GFT_LAUNCH(k_series3_rec<SERIES_LOG>, grid, block, p.lds, st, x, y, res, d, p.tc, p.selems, g); break;
        default: throw std::runtime_error("series3: no such operation at rank 3");
    }
}

}  // namespace gft
