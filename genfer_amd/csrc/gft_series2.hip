// Batched bivariate series (gft_series.hpp, "rank 2"): the planner and the launches of gft_series2_mul / div / exp / log / compose /
// corr / compose_adj, and pow's sequence of mul launches, for F64 and (the first five and pow) for Interval<F64> (the element width w of the entry point: SeriesPlanes).  The kernels
// are in gft_series2_kernels.hpp; gfx950 only.
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
// compose's lanes count mul's output pairs of the full shape, in whole waves up to 512 (measured: S2_COMPOSE_LANES).  pow has no
// kernel of its own beside the writer of the unit item.
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
    granted = S2_BUDGET;
    const void* const* ks = w == 2 ? ki : kf;
    const size_t nk = w == 2 ? sizeof(ki) / sizeof(*ki) : sizeof(kf) / sizeof(*kf);
    for (size_t i = 0; i < nk; ++i)
        if (hipFuncSetAttribute(ks[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)S2_BUDGET) != hipSuccess) {
            (void)hipGetLastError();  // no stale error for the caller's next HIP call
            granted = S2_BUDGET_PLAIN;
            break;
        }
    return granted;
}

// the unit item [[1, 0, ...], [0, ...], ...] of pow: its first factor (one item of one coefficient) and the whole result of e == 0
// (an interval item: [1,1] and [0,0], both planes `plane` apart)
template <class E>
__global__ __launch_bounds__(256) void k_series2_unit(double* res, size_t plane, size_t rr, unsigned n0, unsigned n1, SeriesBatch b) {
    const SeriesOff o = series_offsets(b, blockIdx.x);
    for (unsigned idx = threadIdx.x; idx < n0 * n1; idx += blockDim.x) {
        const unsigned k0 = idx / n1, k1 = idx - k0 * n1;
        E::st(res, plane, o.r + (size_t)k0 * rr + k1, idx == 0 ? E::one() : E::zero());
    }
}

unsigned s2_threads(unsigned work, unsigned most = 256) { return work <= 64 ? 64u : std::min(most, (work + 63) / 64 * 64); }
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
        p.threads = s2_threads((N + 1) / 2);
        p.srows = 0;
        p.lds = ((size_t)d.nx0 * d.nx1 + (size_t)d.ny0 * d.ny1) * elem;
        return p;
    }
    if (op == SERIES_COMPOSE || op == SERIES_COMPOSE_ADJ) {
        const bool adj = op == SERIES_COMPOSE_ADJ;
        const unsigned A = adj ? d.nx0 * d.nx1 : N;  // of an array taking turns: the composition's shape (compose_adj: gh's)
        const size_t rows = (size_t)2 * A * elem, all = rows + (size_t)d.ny0 * d.ny1 * elem;
        p.threads = s2_threads((A + 1) / 2, adj ? S2_ADJ_LANES : S2_COMPOSE_LANES);
        p.srows = 0;
        p.glds = all <= S2_BUDGET_PLAIN || all <= s2_budget(w);
        p.lds = p.glds ? all : rows;
        return p;
    }
    const unsigned a0 = op == SERIES_DIV ? d.ny0 : d.nx0, a1 = op == SERIES_DIV ? d.ny1 : d.nx1;
    const size_t resident = ((size_t)a0 * a1 + N) * elem, row = (size_t)d.n1 * elem;
    unsigned terms = std::min(d.n0, a0) - 1;  // of the longest j range (log's starts at 1: one term fewer while k < nx0)
    if (op == SERIES_LOG && d.n0 <= a0) terms = d.n0 >= 2 ? d.n0 - 2 : 0;
    p.threads = s2_threads(N);
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

size_t series2_pow_workspace(unsigned items, const Series2Dims& d, int w) { return (size_t)w * (3 * (size_t)items * d.n0 * d.n1 + 1); }

namespace {

template <class E>
void s2_pow(hipStream_t st, const double* x, unsigned e, double* res, const Series2Dims& d, const SeriesBatch& g, double* ws, const SeriesPlanes& pl) {
    if (g.items == 0) return;
    const unsigned N = d.n0 * d.n1;
    if (e == 0) {
        GFT_LAUNCH(k_series2_unit<E>, dim3(g.items), dim3(s2_threads(N)), 0, st, res, pl.r, d.rr, d.n0, d.n1, g);
        return;
    }
    // three workspace arrays of items * N elements each, whatever the compact shape of the items in it, and the unit item; plane-major:
    // the upper bounds of everything in the workspace lie `wp` doubles behind the lower ones
    const size_t arr = (size_t)g.items * N, wp = 3 * arr + 1;
    double* spare[2] = {ws + arr, ws + 2 * arr};
    int nspare = 2;
    double* unit = ws + 3 * arr;
    SeriesBatch one;
    one.nd = 0;
    one.items = 1;
    GFT_LAUNCH(k_series2_unit<E>, dim3(1), dim3(64), 0, st, unit, wp, (size_t)1, 1u, 1u, one);
    // the operand, read once through its strides: base = x as compact items of (nx0, nx1)
    double* base = ws;
    unsigned lb0 = d.nx0, lb1 = d.nx1;
    {
        CopyGeom c;
        int k = 0;
        if (E::W == 2) c.ext[k] = 2, c.ss[k] = pl.x, c.ds[k] = wp, ++k;
        size_t cs = (size_t)lb0 * lb1;
        for (int a = g.nd - 1; a >= 0; --a) {
            c.ext[k + a] = g.ext[a];
            c.ss[k + a] = g.xs[a];
            c.ds[k + a] = cs;
            cs *= g.ext[a];
        }
        k += g.nd;
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
        SeriesPlanes wpl;
        wpl.w = E::W;
        if (E::W == 2) wpl.x = wpl.y = wp, wpl.r = last ? pl.r : wp;
        series2_launch(st, SERIES_MUL, series2_plan(SERIES_MUL, m, E::W), a, b, out, m, w, 0, wpl);
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

}  // namespace

void series2_pow(hipStream_t st, const double* x, unsigned e, double* res, const Series2Dims& d, const SeriesBatch& g, double* ws,
                 const SeriesPlanes& pl) {
    if (pl.w == 2) s2_pow<EIv>(st, x, e, res, d, g, ws, pl);
    else s2_pow<EF64>(st, x, e, res, d, g, ws, pl);
}

}  // namespace gft
