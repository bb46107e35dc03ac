// The fused negative-binomial observation on caller-owned device tensors (gft_series_observe_negbinomial / gft_series2_observe_negbinomial
// and their gfti_ twins) and the Lah row it sums with (gft_series_lah_row / gfti_series_lah_row): what the evaluator runs for
// `observe k ~ NegBinomial(X, p)` (generating_function.rs:712-751) -- order + 1 passes of the scaling substitution x_v := p * x_v
// (subst_var's power table, mt:555-567), the product with (p * x + p * x_v)^i through Mul's dispatcher (nothing at i = 0, mul_linear
// at i = 1, the general product from i = 2), the scaling by the row's entry, the accumulation and a derivative.  include/gftaylor.h
// states the loops.  gfx950 only, -ffp-contract=off as the rest; one launch per call, nothing travels through global memory between
// the passes, and the host never waits.
//
// The work is LINES along the axis the observation acts on, as the chain's (gft_series_observe_chain.hip): of a rank-2 item only the
// first min(other axis, degree_p1) lines reach the result.  A line reads degree_p1 + order coefficients of the operand.
//
//   form A  lines with degree_p1 + order <= 64: one wave per line, four lines per workgroup, grid-stride over the lines.  A lane owns
//           D[j], pf[j], sum[j] and P_i[j] for all passes in registers; the product of pass i reads S[j - t] and P_i[t] across lanes
//           (ds_bpermute, t <= min(i, degree_p1 - 1)).  No LDS, no barrier.
//   form B  longer lines: one workgroup of up to 512 lanes per line, D, S and P_i in LDS ((3 * degree_p1 + order) elements: within
//           the 64 KB every kernel may have, by SERIES_NEGBIN_MAX), the sum in the registers of the owning threads,
//           gft::lds_barrier() between the phases of a pass.
//
// Cross-lane reads, not an LDS staging, in form A: a staged S and P_i would cost the same two DS operations per term (a ds_read
// each, where the ds_bpermute pair is) plus a ds_write per pass and (degree_p1 + order + degree_p1) elements of LDS per wave, which
// at 64 coefficients of intervals is 3 KB a wave and would cap the waves of a CU below what the registers allow.
//
// The Lah row: one wave per item while order + 1 <= 64 (lane i owns entry i, the previous entry comes from lane i - 1), else one
// workgroup per item with two rows in LDS taking turns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gft_elem.hpp"
#include "gft_launch.hpp"
#include "gft_series.hpp"
#include "gft_series_observe_negbinomial_kernels.hpp"

namespace gft {

namespace {

constexpr unsigned ONB_MAX_BLOCKS = 1u << 16;  // of the x dimension; every kernel is grid-stride

template <class E>
int observe_negbinomial(hipStream_t st, const double* a, const double* x, const double* p, const double* ls, double* res, const ObsNegbin& q,
                        const ObsNegbinP& sp, const SeriesBatch& g, const SeriesPlanes& pl, const double* tab, size_t tab_plane, int force) {
    const size_t lines = (size_t)g.items * q.lines;
    const int form = q.len <= 64 && force != SERIES_FORM_B ? SERIES_FORM_A : SERIES_FORM_B;
    if (lines == 0) return form;
    if (form == SERIES_FORM_A) {
        const size_t blocks = (lines + ONB_THREADS_A / 64 - 1) / (ONB_THREADS_A / 64);
        GFT_LAUNCH(k_obs_negbin_wave<E>, dim3((unsigned)std::min<size_t>(blocks, ONB_MAX_BLOCKS)), dim3(ONB_THREADS_A), 0, st, a, pl.x, x, pl.y, p, sp, ls,
                   pl.s, res, pl.r, q, tab, tab_plane, g);
        return form;
    }
    const unsigned pad = q.len + 2 * q.degree_p1;  // D, S and P behind each other; the planes of an interval `pad` apart
    GFT_LAUNCH(k_obs_negbin_lds<E>, dim3((unsigned)std::min<size_t>(lines, ONB_MAX_BLOCKS)), dim3(series_threads(q.degree_p1, ONB_THREADS_B)),
               (size_t)E::W * pad * sizeof(double), st, a, pl.x, x, pl.y, p, sp, ls, pl.s, res, pl.r, q, tab, tab_plane, g, pad);
    return form;
}

template <class E>
int lah_row(hipStream_t st, const double* p, double* res, unsigned order, const SeriesBatch& g, const SeriesPlanes& pl, int force) {
    const int form = order + 1 <= 64 && force != SERIES_FORM_B ? SERIES_FORM_A : SERIES_FORM_B;
    if (g.items == 0) return form;
    if (form == SERIES_FORM_A) {
        const size_t blocks = ((size_t)g.items + ONB_THREADS_A / 64 - 1) / (ONB_THREADS_A / 64);
        GFT_LAUNCH(k_lah_row_wave<E>, dim3((unsigned)std::min<size_t>(blocks, ONB_MAX_BLOCKS)), dim3(ONB_THREADS_A), 0, st, p, pl.x, res, pl.r, order, g);
        return form;
    }
    const unsigned pad = order + 1;
    GFT_LAUNCH(k_lah_row_lds<E>, dim3(std::min<unsigned>(g.items, ONB_MAX_BLOCKS)), dim3(series_threads(pad, ONB_THREADS_B)),
               (size_t)2 * E::W * pad * sizeof(double), st, p, pl.x, res, pl.r, order, g, pad);
    return form;
}

}  // namespace

int series_observe_negbinomial(hipStream_t st, const double* a, const double* x, const double* p, const size_t* pstrides, size_t pplane, const double* ls,
                               double* res, const Series2Dims& d, int var, bool rank2, unsigned order, unsigned degree_p1, const SeriesBatch& g,
                               const SeriesPlanes& pl, const double* tab, size_t tab_plane, int force) {
    ObsNegbin q;
    const bool rows = rank2 && var == 0;  // the lines run along axis -2: one per column
    q.len = degree_p1 + order;
    q.lines = rank2 ? std::min(rows ? d.nx1 : d.nx0, degree_p1) : 1;
    q.order = order, q.degree_p1 = degree_p1, q.columns = rows && q.lines > 1;
    q.xline = rows ? 1 : d.xr, q.xel = rows ? d.xr : 1;
    q.rline = rows ? 1 : d.rr, q.rel = rows ? d.rr : 1;
    ObsNegbinP sp;
    sp.plane = pplane;
    for (int i = 0; i < IMAXD; ++i) sp.st[i] = i < g.nd ? pstrides[i] : 0;
    return pl.w == 2 ? observe_negbinomial<EIv>(st, a, x, p, ls, res, q, sp, g, pl, tab, tab_plane, force)
                     : observe_negbinomial<EF64>(st, a, x, p, ls, res, q, sp, g, pl, tab, tab_plane, force);
}

int series_lah_row(hipStream_t st, const double* p, double* res, unsigned order, const SeriesBatch& g, const SeriesPlanes& pl, int force) {
    return pl.w == 2 ? lah_row<EIv>(st, p, res, order, g, pl, force) : lah_row<EF64>(st, p, res, order, g, pl, force);
}

}  // namespace gft
