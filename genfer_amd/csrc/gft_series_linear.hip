// The batched affine substitutions on caller-owned device tensors (gft_series_mul_linear / gft_series_compose_linear, their rank-2
// and gfti_ twins): what the reference runs wherever a series is multiplied by, or a variable replaced with, c + m * x_w -- mul_linear
// (mt:611-623) and subst_var's two linear paths (the power table of mt:557-565 for c == 0 on the replaced variable itself, else the
// Horner loop of mt:569-579 with mul_linear as its product).  include/gftaylor.h states the loops.  Every item carries its own c and m;
// the only data-dependent branch is the per-item test c == 0, made on the device.  gfx950 only, -ffp-contract=off as the rest; one
// launch per call, nothing travels through global memory between the steps, and the host never waits.
//
// The work is LINES along the axis w of the affine series.  A step of the Horner loop is a two-tap recurrence on the line
// (out[j] = res[j-1] * m + c * res[j]) and a slice of f added to its low end.  Where w is the replaced variable, every index of the
// other axis is an independent line and a slice is one coefficient; else an item is one line and a slice a row or column of f.
//
//   mul_linear      one streaming grid-stride kernel, a thread per coefficient of the result
//   compose, form A lines of at most 64 coefficients (n_w <= 64): one wave per line, four lines per workgroup, grid-stride.  A lane
//                   owns position j for the whole loop in registers and reads res[j-1] from the previous lane.  No LDS, no barrier.
//   compose, form B longer lines: one workgroup per line, two line buffers in LDS taking turns with gft::lds_barrier() between the
//                   steps (2 * n_w elements: 64 KB at both limits).
// The power form is a branch per item inside the same launch.  Lines along axis -2 of a rank-2 item are strided in memory: the loads
// and stores go through the row stride as they are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gft_elem.hpp"
#include "gft_launch.hpp"
#include "gft_series.hpp"
#include "gft_series_linear_kernels.hpp"

namespace gft {

namespace {

constexpr unsigned LIN_MAX_BLOCKS = 1u << 16;  // of the x dimension; every kernel is grid-stride

template <class E>
int linear(hipStream_t st, int op, const double* a, const double* c, const double* m, double* res, const LinCall& q, const SeriesBatch& g,
           const SeriesPlanes& pl, int force) {
    if (op == SERIES_MUL_LINEAR) {
        const size_t total = (size_t)g.items * q.lines * q.n, blocks = (total + LIN_THREADS_A - 1) / LIN_THREADS_A;
        GFT_LAUNCH(k_lin_mul<E>, dim3((unsigned)std::min<size_t>(blocks, LIN_MAX_BLOCKS)), dim3(LIN_THREADS_A), 0, st, a, pl.x, c, pl.y, m, pl.s, res,
                   pl.r, q, g);
        return SERIES_NONE;
    }
    const size_t lines = (size_t)g.items * q.lines;
    const int form = q.n <= 64 && force != SERIES_FORM_B ? SERIES_FORM_A : SERIES_FORM_B;
    if (form == SERIES_FORM_A) {
        const size_t blocks = (lines + LIN_THREADS_A / 64 - 1) / (LIN_THREADS_A / 64);
        GFT_LAUNCH(k_lin_compose_wave<E>, dim3((unsigned)std::min<size_t>(blocks, LIN_MAX_BLOCKS)), dim3(LIN_THREADS_A), 0, st, a, pl.x, c, pl.y, m, pl.s,
                   res, pl.r, q, g);
        return form;
    }
    GFT_LAUNCH(k_lin_compose_lds<E>, dim3((unsigned)std::min<size_t>(lines, LIN_MAX_BLOCKS)), dim3(series_threads(q.n, LIN_THREADS_B)),
               (size_t)2 * E::W * q.n * sizeof(double), st, a, pl.x, c, pl.y, m, pl.s, res, pl.r, q, g, q.n);
    return form;
}

}  // namespace

int series_linear(hipStream_t st, int op, const double* a, const double* c, const double* m, double* res, const Series2Dims& d, int var, int wvar,
                  const SeriesBatch& g, const SeriesPlanes& pl, int force) {
    // (axis 0: the rows, stride d.xr / d.rr; axis 1: the unit-stride axis; a rank-1 call is var == wvar == 1 on a one-row item)
    const unsigned nx[2] = {d.nx0, d.nx1}, n[2] = {d.n0, d.n1};
    const size_t xs[2] = {d.xr, 1}, rs[2] = {d.rr, 1};
    const int w = op == SERIES_MUL_LINEAR ? var : wvar, o = 1 - w;
    LinCall q;
    q.lines = n[o], q.n = n[w];
    q.rline = rs[o], q.rel = rs[w];
    q.xel = xs[w];
    if (op == SERIES_MUL_LINEAR || w == var) {
        q.live = nx[o], q.xline = xs[o];
        q.slen = op == SERIES_MUL_LINEAR ? nx[w] : 1;
        q.slices = op == SERIES_MUL_LINEAR ? 1 : nx[w];
        q.xslice = xs[w];
        q.power = op != SERIES_MUL_LINEAR;
    } else {
        q.live = 1, q.xline = 0;
        q.slen = nx[w], q.slices = nx[var], q.xslice = xs[var];
        q.power = 0;
    }
    return pl.w == 2 ? linear<EIv>(st, op, a, c, m, res, q, g, pl, force) : linear<EF64>(st, op, a, c, m, res, q, g, pl, force);
}

}  // namespace gft
