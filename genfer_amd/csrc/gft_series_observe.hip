// Batched observation ops on caller-owned device tensors (gft_series_* / gft_series2_* derivative, taylor_expansion_of_coeff,
// shift_down, evaluate_all_one and their gfti_ twins): the reference's derivative (mt:457-481), taylor_expansion_of_coeff
// (mt:484-509), shift_down (mt:514-536) and evaluate_all_one (mt:583-586) per item, in its operation order.  gfx950 only,
// -ffp-contract=off as the rest.  Every kernel is a template over the element functor (EF64, EIv) and indexes the grid along x
// only, grid-stride, so the number of items is bounded by the 2^31 - 1 of the host side alone.
//
// An item is n0 rows of n1 coefficients (rank 1: n0 == 1), rows `xr` elements apart, unit stride along a row.
//
//   k_obs_scale      derivative / taylor_expansion_of_coeff: one lane per output element, lanes consecutive along the row, one
//                    factor per slice from the (op, k, len) table of k_factor_table.
//   k_obs_shift_cols shift_down along axis 0 of items with n1 > 1: one lane per output element; the lanes of row 0 sum their
//                    column in ascending row order from 0.0 (ndarray's slab-by-slab sum_axis), consecutive lanes are
//                    consecutive columns.
//   k_obs_rows       the sums along the unit-stride axis: eight lanes own a row, so a wave holds eight rows and every load of
//                    the wave is eight 64-byte segments.  FOLD8 (shift_down at rank 2 along axis 1, or along axis 0 of a
//                    one-column item): lane u owns the partial sum p[u] of ndarray's unrolled_fold over whole groups of eight,
//                    the pairs p[u] + p[u+4] are formed by the lanes 0..3, and the chain
//                    (((0+(p0+p4))+(p1+p5))+(p2+p6))+(p3+p7), then the tail in order.  SEQ (rank-1 shift_down,
//                    evaluate_all_one): the lanes walk the row in groups of eight and every lane runs the one chain
//                    0.0 + x[0] + x[1] + ... over the group's values read from its neighbours, which keeps the loads coalesced
//                    and needs no LDS staging.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gft_elem.hpp"
#include "gft_launch.hpp"
#include "gft_series.hpp"
#include "gft_series_observe_kernels.hpp"

namespace gft {

namespace {

constexpr unsigned OBS_MAX_BLOCKS = 1u << 16;  // of the x dimension; the loops are grid-stride

unsigned obs_blocks(size_t work) {
    const size_t b = (work + OBS_THREADS - 1) / OBS_THREADS;
    return (unsigned)std::min<size_t>(std::max<size_t>(b, 1), OBS_MAX_BLOCKS);
}

template <class E>
void observe(hipStream_t st, int op, const double* x, double* res, const Series2Dims& d, int var, unsigned k, const SeriesBatch& g,
             const SeriesPlanes& pl, const double* tab, size_t tab_plane, bool rank2) {
    if (g.items == 0) return;
    if (op == SERIES_DERIVATIVE || op == SERIES_COEFF) {
        const unsigned k0 = var == 0 ? k : 0, k1 = var == 0 ? 0 : k;
        const dim3 grid(obs_blocks((size_t)g.items * d.n0 * d.n1)), block(OBS_THREADS);
        if (op == SERIES_DERIVATIVE)
            GFT_LAUNCH((k_obs_scale<E, false>), grid, block, 0, st, x, pl.x, d.xr, res, pl.r, d.rr, d.n0, d.n1, k0, k1, var, tab, tab_plane, g);
        else
            GFT_LAUNCH((k_obs_scale<E, true>), grid, block, 0, st, x, pl.x, d.xr, res, pl.r, d.rr, d.n0, d.n1, k0, k1, var, tab, tab_plane, g);
        return;
    }
    ObsRows q;
    bool fold8 = false;
    if (op == SERIES_EVAL_ONE) {  // one chain over the item in row-major order
        q.rows = 1;
        q.inner = d.nx1;
        q.flat = d.nx0 == 1 || d.xr == d.nx1;  // (contiguous rows: element e is at e)
        q.xrow = 0, q.xes = d.xr, q.rrow = 0, q.res_es = 0;
        q.cnt = d.nx0 * d.nx1;
        q.k = 0, q.m = 1, q.whole = 1;
    } else {  // SERIES_SHIFT_DOWN
        const unsigned len = var == 0 ? d.nx0 : d.nx1;
        const int whole = len == k + 1;
        const unsigned cnt = whole ? len : k;
        if (var == 0 && d.nx1 > 1) {  // ascending over the rows, per column
            GFT_LAUNCH(k_obs_shift_cols<E>, dim3(obs_blocks((size_t)g.items * d.n0 * d.n1)), dim3(OBS_THREADS), 0, st, x, pl.x, d.xr, res, pl.r,
                       d.rr, d.n0, d.n1, k, cnt, whole, g);
            return;
        }
        fold8 = rank2;  // ndarray's sum_axis: the 8-way fold along a unit-stride axis of a rank-2 array, ascending at rank 1
        q.cnt = cnt, q.k = k, q.whole = whole;
        if (var == 0) {  // a one-column item: its column is the "row"
            q.rows = 1, q.inner = 1, q.flat = 0;
            q.xrow = 0, q.xes = d.xr, q.rrow = 0, q.res_es = d.rr;
            q.m = d.n0;
        } else {
            q.rows = d.nx0, q.inner = d.nx1, q.flat = 1;
            q.xrow = d.xr, q.xes = 0, q.rrow = d.rr, q.res_es = 1;
            q.m = d.n1;
        }
    }
    const size_t rows = (size_t)g.items * q.rows;
    const dim3 grid(obs_blocks(rows * 8)), block(OBS_THREADS);
    if (fold8) GFT_LAUNCH((k_obs_rows<E, true>), grid, block, 0, st, x, pl.x, res, pl.r, q, g);
    else GFT_LAUNCH((k_obs_rows<E, false>), grid, block, 0, st, x, pl.x, res, pl.r, q, g);
}

}  // namespace

void series_observe(hipStream_t st, int op, const double* x, double* res, const Series2Dims& d, int var, unsigned k, const SeriesBatch& g,
                    const SeriesPlanes& pl, const double* tab, size_t tab_plane, bool rank2) {
    if (pl.w == 2) observe<EIv>(st, op, x, res, d, var, k, g, pl, tab, tab_plane, rank2);
    else observe<EF64>(st, op, x, res, d, var, k, g, pl, tab, tab_plane, rank2);
}

}  // namespace gft
