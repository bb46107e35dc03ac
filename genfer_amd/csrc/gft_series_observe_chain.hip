// The fused Poisson observation chain on caller-owned device tensors (gft_series_observe_chain / gft_series2_observe_chain and their
// gfti_ twins): what the evaluator runs for `observe k ~ Poisson(lambda * X)` (generating_function.rs:678-711), nsteps nested steps
// of derivative(v, 1), truncation to d_t, the factor var(v, x, d_t) through mul_linear (mt:611-623; none for a continuous rate) and
// the step's constant, each step one degree lower than the one before: d_t = degree_p1 + (nsteps - 1 - t).  include/gftaylor.h states
// the loops.  gfx950 only, -ffp-contract=off as the rest; one launch per call, nothing travels through global memory between the
// steps, and the host never waits.
//
// The work is LINES along the axis the chain acts on: every other index of an item is carried along, and of a rank-2 item only the
// first min(other axis, degree_p1) lines can reach the result (the truncation of every step cuts the others), so only those run.
// The shape rule degree_p1 + nsteps <= L_0 makes every step full: it reads d_t + 1 coefficients and writes d_t.
//
//   form A  lines of at most 64 coefficients: one wave per line, four lines per workgroup, grid-stride over the lines.  A lane owns
//           position kv for the whole chain in registers; src[kv + 1] is read from the next lane, D[kv - 1] from the previous one.
//           No LDS, no barrier.  The lane's factor ff[kv] is read once; the item's x and the step's c are wave-uniform.
//   form B  longer lines: one workgroup per line, two line buffers in LDS taking turns with gft::lds_barrier() between the steps
//           (2 * (L_0 - 1) elements: below 64 KB at both limits).  A thread's factors are read once where it owns one position.
//
// Lines along axis -2 of a rank-2 item are strided in memory: the first step's loads (and the last step's stores) go through the row
// stride as they are, neither form stages the item through LDS first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gft_elem.hpp"
#include "gft_launch.hpp"
#include "gft_series.hpp"
#include "gft_series_observe_chain_kernels.hpp"

namespace gft {

namespace {

constexpr unsigned OBC_MAX_BLOCKS = 1u << 16;  // of the x dimension; both kernels are grid-stride over the lines

template <class E>
int observe_chain(hipStream_t st, const double* a, const double* x, const double* cs, double* res, const ObsChain& q, const SeriesBatch& g,
                  const SeriesPlanes& pl, const double* tab, size_t tab_plane, int force) {
    const size_t lines = (size_t)g.items * q.lines;
    const int form = q.len <= 64 && force != SERIES_FORM_B ? SERIES_FORM_A : SERIES_FORM_B;
    if (lines == 0) return form;
    if (form == SERIES_FORM_A) {
        const size_t blocks = (lines + OBC_THREADS_A / 64 - 1) / (OBC_THREADS_A / 64);
        GFT_LAUNCH(k_obs_chain_wave<E>, dim3((unsigned)std::min<size_t>(blocks, OBC_MAX_BLOCKS)), dim3(OBC_THREADS_A), 0, st, a, pl.x, x, pl.y, cs, pl.s,
                   res, pl.r, q, tab, tab_plane, g);
        return form;
    }
    const unsigned pad = q.degree_p1 + q.nsteps - 1;  // d_0, the longest line a step writes: at most L_0 - 1
    GFT_LAUNCH(k_obs_chain_lds<E>, dim3((unsigned)std::min<size_t>(lines, OBC_MAX_BLOCKS)), dim3(series_threads(pad, OBC_THREADS_B)),
               (size_t)2 * E::W * pad * sizeof(double), st, a, pl.x, x, pl.y, cs, pl.s, res, pl.r, q, tab, tab_plane, g, pad);
    return form;
}

}  // namespace

int series_observe_chain(hipStream_t st, const double* a, const double* x, const double* cs, double* res, const Series2Dims& d, int var, bool rank2,
                         unsigned nsteps, unsigned degree_p1, const SeriesBatch& g, const SeriesPlanes& pl, const double* tab, size_t tab_plane,
                         int force) {
    ObsChain q;
    const bool rows = rank2 && var == 0;  // the lines run along axis -2: one per column
    q.len = rows ? d.nx0 : d.nx1;
    q.lines = rank2 ? std::min(rows ? d.nx1 : d.nx0, degree_p1) : 1;
    q.nsteps = nsteps, q.degree_p1 = degree_p1, q.discrete = x != nullptr;
    q.xline = rows ? 1 : d.xr, q.xel = rows ? d.xr : 1;
    q.rline = rows ? 1 : d.rr, q.rel = rows ? d.rr : 1;
    return pl.w == 2 ? observe_chain<EIv>(st, a, x, cs, res, q, g, pl, tab, tab_plane, force)
                     : observe_chain<EF64>(st, a, x, cs, res, q, g, pl, tab, tab_plane, force);
}

}  // namespace gft
