// Batched univariate series on caller-owned device tensors (gft_series_mul / div / exp / log / compose / pow): B independent truncated power
// series per call, the last axis of every operand is the series, the leading axes are the batch.  Per item the results are
// the reference's GENERAL algorithms in its operation order (mul_1d mt:972-982, div mt:1162-1192 at one axis, exp_1d
// mt:1271-1283, log_1d mt:1319-1333), multiply and add rounded separately.  None of the data-dependent shortcuts of the
// operator wrappers is taken (Mul: zero / one / constant / linear, mt:1020-1070; Div: one / constant, mt:1204-1213): a batch
// cannot branch per item on the host, and the result of an item must not depend on what else is in the batch.
// compose is subst_var's Horner loop (mt:574-578) and pow the square-and-multiply of mt:441-450, both over that general product at
// the compact lengths min(la + lb - 1, n) of sum_shape (mt:150-170).  compose costs about nf * n^2 / 2 multiply-adds per item, all
// of them on one workgroup at most.
//
// The host side (gft_series_args.hpp, gft_api_series.inc) validates, collapses the batch axes into a SeriesBatch and joins the streams; this
// file's planner picks a form and gft_series.hip (div form B: gft_div2d.hip) launches it on the library's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "gft_interop.hpp"  // interop_copy
#include "gft_series_args.hpp"

namespace gft {

// (SeriesOp, the limits, SeriesPlanes, SeriesBatch, SeriesItem and Series2Dims: gft_series_args.hpp, the HIP-free argument layer)
// A: one lane is one series, rows staged in LDS.  B: one wave / workgroup is one series (mul, div, compose); for exp / log the
// lane-per-series loop of form A over a transposed global workspace.  pow is a sequence of mul launches, each planned by itself.
enum SeriesForm { SERIES_NONE = 0, SERIES_FORM_A = 1, SERIES_FORM_B = 2 };

// The form a call takes.  force: 0 = by the thresholds, SERIES_FORM_A = form A whenever the rows fit its LDS budget,
// SERIES_FORM_B = never form A (gft_set_option("series_form")).
// `w`, `elem`: the planes per tensor and what they hold (SeriesElem: Interval<F64> and BigFloat are both w == 2).
int series_plan(int op, unsigned items, unsigned n, int force, int w = 1, int elem = SERIES_ELEM_BY_WIDTH);
// doubles of device workspace the call needs (form B of exp / log: the transposed operand and result, each of w planes), else 0.
// Not for SERIES_POW (series_pow_workspace).
size_t series_workspace(int op, int form, unsigned items, unsigned nx, unsigned n, int w = 1);
// Launches the call on `st`.  `y`: the second operand of mul / div / compose (x is f, y is g); for exp / log the seeds or nullptr
// (seeds formed on the device by the HIP device library's exp / log).  `ws`: series_workspace() doubles.  Not for SERIES_POW.
// `pl`: the planes, their strides and the element kind (pl.elem == SERIES_ELEM_BIGFLOAT: rank 1's six arithmetic ops only).
// corr and compose_adj: the result is the SHORT side, n <= nx, and series_plan takes the long side nx (the rows held in LDS).
void series_launch(hipStream_t st, int op, int form, const double* x, unsigned nx, const double* y, unsigned ny, double* res,
                   unsigned n, const SeriesBatch& g, double* ws, const SeriesPlanes& pl = SeriesPlanes());
// pow at every rank (gft[i]_series_pow, _series2_pow, _series3_pow): x^e on `st` by the steps of series_pow_steps
// (gft_series_args.hpp).  x is copied once through its strides into the workspace, every product but the last is the rank's
// SERIES_MUL launch (series_launch, series2_launch, series3_launch, each planned by itself) on compact workspace items, the last one
// writes all of n through the result's strides.  e == 0 only writes the unit item.  `ws`: series_pow_workspace() doubles, plane-major
// -- three arrays of items * n0 * n1 * n2 and the unit item [1.0], and the upper bounds of all of that behind the lower ones.
// `force` as for series_plan (rank 1 only).  Returns what gft_series_last_form() reports: at rank 1 the form of the last product
// (SERIES_NONE for e == 0), above it SERIES_FORM_B.
size_t series_pow_workspace(unsigned items, const unsigned* n, int w = 1);
int series_pow(hipStream_t st, int rank, const double* x, unsigned e, double* res, const SeriesItem& it, const SeriesBatch& g, double* ws,
               int force, const SeriesPlanes& pl = SeriesPlanes());
// lanes of a one-workgroup-per-item launch: one wave up to 64 units of parallel work, else whole waves up to `most`
inline unsigned series_threads(unsigned work, unsigned most = 256) { return work <= 64 ? 64u : std::min(most, (work + 63) / 64 * 64); }
// form B of div: k_div_1d_wave / k_div_1d with blockIdx.x as the item (gft_div2d.hip)
void series_div_rows(hipStream_t st, const double* x, unsigned nx, const double* y, unsigned ny, double* res, unsigned n,
                     const SeriesBatch& g, const SeriesPlanes& pl = SeriesPlanes());

// ---- rank 2: batched bivariate series (gft_series2_* on F64, gfti_series2_* on Interval<F64>: mul / div / exp / log / compose / pow) --
// The last TWO axes of every operand are one item's coefficient array: axis -2 is variable 0 (rows, any non-negative stride), axis
// -1 variable 1 (unit stride).  Per item the results are the reference's general recursion over axis 0 (mul mt:984-1012, div
// mt:1162-1192, exp mt:1285-1317, log mt:1335-1386) with the univariate loops above on the rows: a row sum mul_1d(a, b) is formed
// from 0.0 first and then added, in ascending j, to the row's accumulator.  One form: one workgroup per item for the whole
// operation, the operands resident in LDS (gft_series2_kernels.hpp); gft_series_last_form() reports SERIES_FORM_B.
// compose is subst_var's Horner loop (mt:569-579) over the rows (var 0) or columns (var 1) of f and pow the square-and-multiply of
// mt:441-450, both over that general product at the compact shapes min(la + lb - 1, n) per axis.  compose costs about
// slices * (n0 * n1)^2 / 4 multiply-adds per item, all of them on one workgroup.
// The geometry of a call of element width w (1: F64, 2: Interval<F64>): lanes per workgroup, scratch rows of n1 elements (div / exp / log: the row sums of one chunk of j), the
// dynamic LDS in bytes, and for compose whether g is resident in LDS.  Throws std::runtime_error where the runtime grants less LDS
// than the resident arrays and one scratch row need.
struct Series2Plan {
    unsigned threads, srows;
    size_t lds;
    bool glds = false;
};
Series2Plan series2_plan(int op, const Series2Dims& d, int w = 1);
// Launches SERIES_MUL / DIV / EXP / LOG / COMPOSE at rank 2 on `st`.  `y`: the divisor / second factor / compose's g (x is f, and
// `var` the variable of f that g replaces); for exp / log the seeds or nullptr.  `pl`: the element width and the plane strides.  Not
// for SERIES_POW (series_pow).  SERIES_CORR and SERIES_COMPOSE_ADJ (w == 1 only): the transposed product and the transposed Horner loop of
// gft_series2_corr / gft_series2_compose_adj, x the long side (g; gh with y = g and `var`), the result the short one.
void series2_launch(hipStream_t st, int op, const Series2Plan& p, const double* x, const double* y, double* res, const Series2Dims& d,
                    const SeriesBatch& g, int var = 0, const SeriesPlanes& pl = SeriesPlanes());

// ---- rank 3: batched trivariate series (gft_series3_* on F64, gfti_series3_* on Interval<F64>: mul / div / exp / log / compose / pow) ---
// The last THREE axes of every operand are one item's coefficient array: axis -3 the slabs and axis -2 the rows (any non-negative
// strides), axis -1 unit stride.  Per item the reference's general recursion over axis 0 at the stored result shape S, an S with
// unit axes being the item without them: Series3Dims (gft_series_args.hpp) says what runs, gft_series3_kernels.hpp how.  One form,
// one workgroup per item; gft_series_last_form() reports SERIES_FORM_B.
// The geometry of a call of element width w (1: F64, 2: Interval<F64>, an LDS element of 16 bytes): lanes per workgroup, the terms per
// chunk of the slab sums (div / exp / log), the scratch in elements and
// the dynamic LDS in bytes.  Throws std::runtime_error where the runtime grants less LDS than the resident arrays and the smallest
// scratch need.
struct Series3Plan {
    unsigned threads, tc = 0, selems = 0;
    size_t lds;
    bool glds = false;  // compose: g is resident in LDS
};
Series3Plan series3_plan(int op, const Series3Dims& d, int w = 1);
// Launches SERIES_MUL / DIV / EXP / LOG at rank 3 on `st`.  `y`: the divisor / second factor; for exp / log the seeds or nullptr.
// `pl`: the element width and the plane strides.
void series3_launch(hipStream_t st, int op, const Series3Plan& p, const double* x, const double* y, double* res, const Series3Dims& d,
                    const SeriesBatch& g, const SeriesPlanes& pl = SeriesPlanes());

// compose at rank 3 (gft_series3_compose): subst_var's Horner loop over the slices of f along `var`, every step series3.mul's product at
// the compact shape, the whole chain one launch on the permuted item of Series3Compose (gft_series_args.hpp).  The plan: lanes, the
// dynamic LDS and whether g is resident in it (else it is read from global memory: every admissible shape runs).
Series3Plan series3_compose_plan(const Series3Compose& c, int w = 1);
void series3_compose_launch(hipStream_t st, const Series3Plan& p, const double* f, const double* g, double* res, const Series3Compose& c,
                            const SeriesBatch& b, const SeriesPlanes& pl = SeriesPlanes());

// ---- the observation ops at ranks 1 and 2 (gft_series_observe.hip) ----------------------------------------------------------------
// op is SERIES_DERIVATIVE / SERIES_COEFF / SERIES_SHIFT_DOWN / SERIES_EVAL_ONE.  `d`: the operand's stored shape (nx0, nx1), row
// stride xr, and the result's (n0, n1), rr (rank 1: nx0 == n0 == 1; evaluate_all_one: n0 == n1 == 1); the axis `var` of the result
// is `k` shorter than the operand's.  `tab`: the k_factor_table factors of (TAB_DERIV | TAB_COEFF, k, len - k), planes tab_plane
// apart (the two scalings only).  `rank2`: the call is gft_series2_* -- ndarray's sum_axis folds a unit-stride axis of a rank-2
// array 8-way and sums everything else in ascending order.  One launch; no workspace.
void series_observe(hipStream_t st, int op, const double* x, double* res, const Series2Dims& d, int var, unsigned k, const SeriesBatch& g,
                    const SeriesPlanes& pl, const double* tab, size_t tab_plane, bool rank2);

// ---- the fused observation chain at ranks 1 and 2 (gft_series_observe_chain.hip) -----------------------------------------------------
// SERIES_OBSERVE_CHAIN: nsteps steps along the axis `var` of the operand `a` (d: its stored shape and row stride, the result's shape
// and row stride), the last one at degree_p1.  `x`: one scalar per item at the batch strides g.ys (planes pl.y apart) or nullptr, the
// continuous form; `cs`: nsteps constants per item at g.ss, unit stride (planes pl.s apart).  `tab`: the k_factor_table factors of
// (TAB_DERIV, 1, L_0 - 1).  `force` as for series_plan: form A (one wave per line) holds up to 64 coefficients on the axis.
// One launch, no workspace; returns the form.
int series_observe_chain(hipStream_t st, const double* a, const double* x, const double* cs, double* res, const Series2Dims& d, int var, bool rank2,
                         unsigned nsteps, unsigned degree_p1, const SeriesBatch& g, const SeriesPlanes& pl, const double* tab, size_t tab_plane,
                         int force);

// ---- the fused negative-binomial observation at ranks 1 and 2, and the Lah row (gft_series_observe_negbinomial.hip) ---------------------
// SERIES_OBSERVE_NEGBINOMIAL: order + 1 passes along the axis `var` of the operand `a` (d as for the chain), the result at degree_p1.
// `x`, `p`: one scalar per item each, x at the batch strides g.ys (planes pl.y apart), p at `pstrides` over the same collapsed axes
// (planes pplane apart); `ls`: order + 1 entries per item at g.ss, unit stride (planes pl.s apart).  `tab`: the k_factor_table
// factors of (TAB_DERIV, 1, at least degree_p1 + order - 1).  `force` as for series_plan: form A (one wave per line) holds up to 64
// coefficients of degree_p1 + order.  One launch, no workspace; returns the form.
int series_observe_negbinomial(hipStream_t st, const double* a, const double* x, const double* p, const size_t* pstrides, size_t pplane, const double* ls,
                               double* res, const Series2Dims& d, int var, bool rank2, unsigned order, unsigned degree_p1, const SeriesBatch& g,
                               const SeriesPlanes& pl, const double* tab, size_t tab_plane, int force);
// SERIES_LAH_ROW: `p` one scalar per item at g.xs (planes pl.x apart), the result order + 1 entries per item at g.rs.  Form A (one
// wave per item) holds rows of up to 64 entries.  One launch; returns the form.
int series_lah_row(hipStream_t st, const double* p, double* res, unsigned order, const SeriesBatch& g, const SeriesPlanes& pl, int force);

// ---- the affine substitutions at ranks 1 and 2 (gft_series_linear.hip) -----------------------------------------------------------------
// SERIES_MUL_LINEAR: a times c + m * x_var; SERIES_COMPOSE_LINEAR: x_var := c + m * x_wvar in f.  d: the operand's stored shape and row
// stride, the result's shape and row stride (rank 1: one row, var == wvar == 1).  `c`, `m`: one scalar per item each at the batch
// strides g.ys / g.ss (planes pl.y / pl.s apart).  `force` as for series_plan: compose's form A (one wave per line) holds up to 64
// coefficients on the axis of wvar.  One launch, no workspace; returns the form (SERIES_NONE for mul_linear, a streaming kernel).
int series_linear(hipStream_t st, int op, const double* a, const double* c, const double* m, double* res, const Series2Dims& d, int var, int wvar,
                  const SeriesBatch& g, const SeriesPlanes& pl, int force);

// the element offsets of item `it` (kernels of gft_series.hip and gft_div2d.hip)
struct SeriesOff {
    size_t x, y, s, r;
};
__device__ inline SeriesOff series_offsets(const SeriesBatch& g, unsigned it) {
    SeriesOff o{0, 0, 0, 0};
    unsigned q = it;
    for (int a = g.nd - 1; a >= 0; --a) {
        const unsigned e = g.ext[a], nq = q / e, k = q - nq * e;
        q = nq;
        o.x += (size_t)k * g.xs[a];
        o.y += (size_t)k * g.ys[a];
        o.s += (size_t)k * g.ss[a];
        o.r += (size_t)k * g.rs[a];
    }
    return o;
}

}  // namespace gft
