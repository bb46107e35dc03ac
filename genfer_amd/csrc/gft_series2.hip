// Batched bivariate series (gft_series.hpp, "rank 2"): the planner and the launches of gft_series2_mul / div / exp / log / compose,
// and pow's sequence of mul launches.  The kernels are in gft_series2_kernels.hpp; gfx950 only, f64 only.
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
// compose's lanes count mul's output pairs of the full shape, in whole waves up to 512 (measured: S2_COMPOSE_LANES).  pow has no
// kernel of its own beside the writer of the unit item.
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

// what the runtime grants the three recurrence kernels and compose with g resident, asked once
size_t s2_budget() {
    static size_t granted = 0;
    if (granted) return granted;
    const void* ks[] = {(const void*)k_series2_rec<SERIES_DIV>, (const void*)k_series2_rec<SERIES_EXP>, (const void*)k_series2_rec<SERIES_LOG>,
                        (const void*)k_series2_compose<true>};
    granted = S2_BUDGET;
    for (const void* k : ks)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S2_BUDGET) != hipSuccess) {
            (void)hipGetLastError();  // no stale error for the caller's next HIP call
            granted = S2_BUDGET_PLAIN;
            break;
        }
    return granted;
}

// the unit item [[1, 0, ...], [0, ...], ...] of pow: its first factor (one item of one coefficient) and the whole result of e == 0
__global__ __launch_bounds__(256) void k_series2_unit(double* res, size_t rr, unsigned n0, unsigned n1, SeriesBatch b) {
    const SeriesOff o = series_offsets(b, blockIdx.x);
    for (unsigned idx = threadIdx.x; idx < n0 * n1; idx += blockDim.x) {
        const unsigned k0 = idx / n1, k1 = idx - k0 * n1;
        res[o.r + (size_t)k0 * rr + k1] = idx == 0 ? 1.0 : 0.0;
    }
}

unsigned s2_threads(unsigned work, unsigned most = 256) { return work <= 64 ? 64u : std::min(most, (work + 63) / 64 * 64); }
// compose: two waves a SIMD on the large items.  Measured on (256, 32, 32) / (256, 64, 64) / (64, 32, 128) items: 256 lanes 1.93 / 67.3 /
// 27.4 ms, 512 lanes 1.23 / 59.0 / 22.0 ms, 1024 lanes 1.23 / 59.9 / 22.5 ms (profiles/r12/series2_compose_lanes.json).
constexpr unsigned S2_COMPOSE_LANES = 512;

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
    if (op == SERIES_COMPOSE) {
        const size_t rows = (size_t)2 * N * sizeof(double), all = rows + (size_t)d.ny0 * d.ny1 * sizeof(double);
        p.threads = s2_threads((N + 1) / 2, S2_COMPOSE_LANES);
        p.srows = 0;
        p.glds = all <= S2_BUDGET_PLAIN || all <= s2_budget();
        p.lds = p.glds ? all : rows;
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
                    const SeriesBatch& g, int var) {
    if (g.items == 0) return;
    const dim3 grid(g.items), block(p.threads);
    switch (op) {
        case SERIES_MUL: GFT_LAUNCH(k_series2_mul, grid, block, p.lds, st, x, y, res, d, g); break;
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

size_t series2_pow_workspace(unsigned items, const Series2Dims& d) { return 3 * (size_t)items * d.n0 * d.n1 + 1; }

void series2_pow(hipStream_t st, const double* x, unsigned e, double* res, const Series2Dims& d, const SeriesBatch& g, double* ws) {
    if (g.items == 0) return;
    const unsigned N = d.n0 * d.n1;
    if (e == 0) {
        GFT_LAUNCH(k_series2_unit, dim3(g.items), dim3(s2_threads(N)), 0, st, res, d.rr, d.n0, d.n1, g);
        return;
    }
    // three workspace arrays of items * N doubles each, whatever the compact shape of the items in it
    const size_t arr = (size_t)g.items * N;
    double* spare[2] = {ws + arr, ws + 2 * arr};
    int nspare = 2;
    double* unit = ws + 3 * arr;
    SeriesBatch one;
    one.nd = 0;
    one.items = 1;
    GFT_LAUNCH(k_series2_unit, dim3(1), dim3(64), 0, st, unit, (size_t)1, 1u, 1u, one);
    // the operand, read once through its strides: base = x as compact items of (nx0, nx1)
    double* base = ws;
    unsigned lb0 = d.nx0, lb1 = d.nx1;
    {
        CopyGeom c;
        size_t cs = (size_t)lb0 * lb1;
        for (int a = g.nd - 1; a >= 0; --a) {
            c.ext[a] = g.ext[a];
            c.ss[a] = g.xs[a];
            c.ds[a] = cs;
            cs *= g.ext[a];
        }
        int k = g.nd;
        c.ext[k] = lb0, c.ss[k] = d.xr, c.ds[k] = lb1, ++k;
        c.ext[k] = lb1, c.ss[k] = 1, c.ds[k] = 1, ++k;
        c.nd = k;
        interop_copy(st, x, base, c);
    }
    double* acc = unit;  // res of mt:441: [[1.0]] for every item until the first product
    unsigned la0 = 1, la1 = 1;
    // a (a0, a1) * b (b0, b1), compact workspace items (`a` may be the one unit item), into `out`: compact at (l0, l1), or (last)
    // the caller's result at all of (n0, n1)
    auto product = [&](const double* a, unsigned a0, unsigned a1, const double* b, unsigned b0, unsigned b1, double* out, unsigned l0, unsigned l1,
                       bool last) {
        Series2Dims m;
        m.nx0 = a0, m.nx1 = a1, m.ny0 = b0, m.ny1 = b1;
        m.n0 = last ? d.n0 : l0, m.n1 = last ? d.n1 : l1;
        m.xr = a1, m.yr = b1, m.rr = last ? d.rr : l1;
        SeriesBatch w = g;
        w.inplace = 0;
        const size_t xi = a == unit ? 0 : (size_t)a0 * a1, yi = (size_t)b0 * b1, ri = (size_t)l0 * l1;
        size_t cs = 1;
        for (int ax = g.nd - 1; ax >= 0; --ax) {
            w.xs[ax] = cs * xi;
            w.ys[ax] = cs * yi;
            w.ss[ax] = 0;
            if (!last) w.rs[ax] = cs * ri;
            cs *= g.ext[ax];
        }
        series2_launch(st, SERIES_MUL, series2_plan(SERIES_MUL, m), a, b, out, m, w);
    };
    while (e > 0) {
        if (e & 1) {
            const bool last = (e >> 1) == 0;
            const unsigned l0 = std::min(la0 + lb0 - 1, d.n0), l1 = std::min(la1 + lb1 - 1, d.n1);
            double* out = last ? res : spare[--nspare];
            product(acc, la0, la1, base, lb0, lb1, out, l0, l1, last);
            if (acc != unit) spare[nspare++] = acc;
            acc = out;
            la0 = l0, la1 = l1;
        }
        e >>= 1;
        if (e > 0) {
            const unsigned l0 = std::min(2 * lb0 - 1, d.n0), l1 = std::min(2 * lb1 - 1, d.n1);
            double* out = spare[--nspare];
            product(base, lb0, lb1, base, lb0, lb1, out, l0, l1, false);
            spare[nspare++] = base;
            base = out;
            lb0 = l0, lb1 = l1;
        }
    }
}

}  // namespace gft
