// The host-side argument layer of the batched series calls (gft[i]_series[2|3]_*): the plain types a call of any rank is described
// and planned with (one SeriesCall in, one SeriesItem out), and everything that is judged about a call without touching device
// state -- the shape rules, the batch, the strides, the result's distinct addresses, the overlap proof and the collapse of the
// batch axes into a SeriesBatch; then what is planned from the shapes alone: the rank-3 item, compose's chain and pow's steps.
// What an operation IS -- its family, its highest rank, its operands' names and roles, its long side, what its result may alias --
// is stated once, in the rows of SERIES_OPS; series_shapes, series_args and the caller's dispatch read the row.  Rules of one op
// (the chain's counts, series_linear_shapes, the observation ops' k, pow's cap on batch axes, corr's and compose_adj's length names)
// stay code, keyed on the op or the family.
// No HIP include: this header compiles with a plain host compiler (tests/series_args_main.cpp replays refusals through it).
// The device side (planners, launches, __device__ helpers) is gft_series.hpp; the caller with the device is gft_api_series.inc.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace gft {

constexpr int IMAXD = 13;  // MAXD + 1: the shape's axes after collapsing, plus the lo / hi plane axis of an interval tensor

enum SeriesOp {
    SERIES_MUL = 0,
    SERIES_DIV = 1,
    SERIES_EXP = 2,
    SERIES_LOG = 3,
    SERIES_COMPOSE = 4,
    SERIES_POW = 5,
    // The transposed product, the adjoint of mul (f64 only): c[i] = 0 + sum_k g[k] * y[k-i], k DESCENDING from min(ng-1, i+ny-1) to i,
    // i < m <= ng -- bit for bit mul_1d(flip(g), y) at index ng-1-i.  x is g (nx = ng: the LONG side), y is y (ny <= ng), n is m.
    SERIES_CORR = 6,
    // The transposed Horner loop, the gradient of compose with respect to f (f64 only): a_0 = gh[0 .. l_0), out[i] = a_i[0],
    // a_{i+1} = corr(a_i, g) at the lengths l_i = min(1 + (nf-1-i)(ng-1), n).  x is gh (nx = n), y is g (ny = ng <= n), n is nf <= nx.
    // One form (B: one workgroup per series for the whole loop).
    SERIES_COMPOSE_ADJ = 7,
    // The observation ops (gft_series_observe.hip): one operand, the result shorter by the order k on the axis they act on.
    // derivative (mt:457-481), taylor_expansion_of_coeff (mt:484-509), shift_down (mt:514-536), evaluate_all_one (mt:583-586).
    SERIES_DERIVATIVE = 8,
    SERIES_COEFF = 9,
    SERIES_SHIFT_DOWN = 10,
    SERIES_EVAL_ONE = 11,
    // The fused Poisson observation chain (gft_series_observe_chain.hip): `nsteps` steps of derivative(v, 1), truncation, the factor
    // var(v, x) (none where x is null: the continuous rate) and the step's constant, per item; x is the operand `a` and the LONG side,
    // y the scalars x (one element per item, as the seeds), cs the constants.  The result has degree_p1 coefficients on the axis.
    SERIES_OBSERVE_CHAIN = 12,
    // The affine substitutions (gft_series_linear.hip, ranks 1 and 2): x is the operand (a / f), y the scalars c and cs the scalars m
    // (one element per item each, as the seeds), the result the LONG side.  mul_linear (mt:611-623): a times c + m * x_var.
    // compose_linear (subst_var's linear paths, mt:555-579): x_var := c + m * x_wvar.
    SERIES_MUL_LINEAR = 13,
    SERIES_COMPOSE_LINEAR = 14,
    SERIES_OP_COUNT,  // (no operation: the length of SERIES_OPS, the table the Python layer's OPS mirrors row by row)
    // The operations behind the table: their rows are SERIES_MORE_OPS.  SERIES_OPS ends with the affine substitutions -- the tests of
    // that layer pin them as the last rows of the Python table, and the two tables are held together row by row -- so an operation
    // added later is stated here, and series_op_row() finds the row of either kind.
    // The fused negative-binomial observation (gft_series_observe_negbinomial.hip; generating_function.rs:731-750): order + 1 passes of
    // the scaling substitution x_v := p * x_v, the product with (p * x + p * x_v)^i, the scaling by the row's entry, the accumulation
    // and a derivative.  x is the operand `a` and the LONG side, y the scalars x and the view `p` the scalars p (one element per item
    // each), cs the row ls with len[2] = order + 1.  Of the chain's family: the result has degree_p1 coefficients on the axis.
    SERIES_OBSERVE_NEGBINOMIAL = SERIES_OP_COUNT + 1,
    // The row of scaled Lah numbers such an observation sums with (generating_function.rs:713-730): x is the scalar p of every item
    // (no series axis: len 1), the result the row of order + 1 entries.  One entry point (gft[i]_series_lah_row): the operand has no
    // rank, and `ranks` below only says that rank 3 keeps its refusal.
    SERIES_LAH_ROW,
    SERIES_OP_END  // (no operation: one past the last of SERIES_MORE_OPS)
};

// One row per SeriesOp.  family: what series_call dispatches on.  ranks: the highest rank the op exists at.  x / y / cs: the
// operands' names in the stride, pointer and overlap messages ("-": the op has no such operand; its view stays the default one,
// about which nothing can be refused).  yrole: y is a second series; the optional seeds (null allowed; their strides travel as
// ss / pl.s); or one scalar per item (its strides travel as ys / pl.y; optional for the chain, whose continuous form has none).
// csrole: cs is the chain's constants or the substitutions' scalar m (either way its strides travel as ss / pl.s).  xlong: x, not
// the result, is the long side.  alias_x / alias_y: the result may be that operand itself, as the same view.
enum SeriesFamily { SERIES_ARITH, SERIES_POWER, SERIES_OBSERVE, SERIES_CHAIN, SERIES_LINEAR };
enum SeriesYRole { SERIES_Y_NONE, SERIES_Y_SERIES, SERIES_Y_SEEDS, SERIES_Y_SCALAR };
enum SeriesCsRole { SERIES_CS_NONE, SERIES_CS_CONSTANTS, SERIES_CS_SCALAR };
struct SeriesOpRow {
    SeriesOp op;
    SeriesFamily family;
    int ranks;
    const char *x, *y, *cs;
    SeriesYRole yrole;
    SeriesCsRole csrole;
    bool xlong, alias_x, alias_y;
};
constexpr SeriesOpRow SERIES_OPS[] = {
    {SERIES_MUL, SERIES_ARITH, 3, "x", "y", "-", SERIES_Y_SERIES, SERIES_CS_NONE, false, true, true},
    {SERIES_DIV, SERIES_ARITH, 3, "x", "y", "-", SERIES_Y_SERIES, SERIES_CS_NONE, false, true, true},
    {SERIES_EXP, SERIES_ARITH, 3, "x", "the seeds", "-", SERIES_Y_SEEDS, SERIES_CS_NONE, false, true, false},
    {SERIES_LOG, SERIES_ARITH, 3, "x", "the seeds", "-", SERIES_Y_SEEDS, SERIES_CS_NONE, false, true, false},
    {SERIES_COMPOSE, SERIES_ARITH, 3, "f", "g", "-", SERIES_Y_SERIES, SERIES_CS_NONE, false, true, true},
    {SERIES_POW, SERIES_POWER, 3, "x", "-", "-", SERIES_Y_NONE, SERIES_CS_NONE, false, true, false},
    // (corr's result may be g itself, compose_adj's gh; neither may be the second operand)
    {SERIES_CORR, SERIES_ARITH, 2, "g", "y", "-", SERIES_Y_SERIES, SERIES_CS_NONE, true, true, false},
    {SERIES_COMPOSE_ADJ, SERIES_ARITH, 2, "gh", "g", "-", SERIES_Y_SERIES, SERIES_CS_NONE, true, true, false},
    {SERIES_DERIVATIVE, SERIES_OBSERVE, 2, "x", "-", "-", SERIES_Y_NONE, SERIES_CS_NONE, true, true, false},
    {SERIES_COEFF, SERIES_OBSERVE, 2, "x", "-", "-", SERIES_Y_NONE, SERIES_CS_NONE, true, true, false},
    {SERIES_SHIFT_DOWN, SERIES_OBSERVE, 2, "x", "-", "-", SERIES_Y_NONE, SERIES_CS_NONE, true, true, false},
    {SERIES_EVAL_ONE, SERIES_OBSERVE, 2, "x", "-", "-", SERIES_Y_NONE, SERIES_CS_NONE, true, true, false},
    // (a chain's result is shorter than its operand: never the same view; a substitution's result is no operand)
    {SERIES_OBSERVE_CHAIN, SERIES_CHAIN, 2, "a", "x", "cs", SERIES_Y_SCALAR, SERIES_CS_CONSTANTS, true, false, false},
    {SERIES_MUL_LINEAR, SERIES_LINEAR, 2, "a", "c", "m", SERIES_Y_SCALAR, SERIES_CS_SCALAR, false, false, false},
    {SERIES_COMPOSE_LINEAR, SERIES_LINEAR, 2, "f", "c", "m", SERIES_Y_SCALAR, SERIES_CS_SCALAR, false, false, false},
};
// the rows of the operations behind SERIES_OP_COUNT, in the enum's order
constexpr SeriesOpRow SERIES_MORE_OPS[] = {
    // (the negative-binomial observation: the chain's family with its own rules and a required x; its fourth operand is SeriesCall::p)
    {SERIES_OBSERVE_NEGBINOMIAL, SERIES_CHAIN, 2, "a", "x", "ls", SERIES_Y_SCALAR, SERIES_CS_CONSTANTS, true, false, false},
    // (one operand, as the observation ops; the result is the long side and never the operand)
    {SERIES_LAH_ROW, SERIES_OBSERVE, 2, "p", "-", "-", SERIES_Y_NONE, SERIES_CS_NONE, false, false, false},
};
constexpr bool series_ops_in_enum_order() {
    for (int i = 0; i < (int)(sizeof(SERIES_OPS) / sizeof(SERIES_OPS[0])); ++i)
        if (SERIES_OPS[i].op != i) return false;
    return true;
}
static_assert(sizeof(SERIES_OPS) / sizeof(SERIES_OPS[0]) == SERIES_OP_COUNT && series_ops_in_enum_order(),
              "SERIES_OPS has one row per SeriesOp, in the enum's order (tests/make_series_refusals.py indexes the ops by position)");
static_assert(sizeof(SERIES_MORE_OPS) / sizeof(SERIES_MORE_OPS[0]) == SERIES_OP_END - SERIES_OBSERVE_NEGBINOMIAL &&
                  SERIES_MORE_OPS[0].op == SERIES_OBSERVE_NEGBINOMIAL && SERIES_MORE_OPS[1].op == SERIES_LAH_ROW,
              "SERIES_MORE_OPS has one row per operation behind SERIES_OP_COUNT, in the enum's order");
// the row of an operation of either table (an op outside both: std::logic_error, a caller's mistake and no refusal)
inline const SeriesOpRow& series_op_row(int op) {
    if (op >= 0 && op < SERIES_OP_COUNT) return SERIES_OPS[op];
    if (op >= SERIES_OBSERVE_NEGBINOMIAL && op < SERIES_OP_END) return SERIES_MORE_OPS[op - SERIES_OBSERVE_NEGBINOMIAL];
    throw std::logic_error("series_op_row: no such operation");
}

constexpr unsigned SERIES_MAX_N = 4096;  // the limit of this first version (form B's mul and div hold a row pair in 64 KB of LDS)
// Interval<F64> series (gfti_series_*): two planes per row, so the same LDS footprints are reached at half the order
constexpr unsigned SERIES_MAX_N_IV = 2048;
constexpr unsigned SERIES2_MAX_ELEMS = 4096;  // n0 * n1 of the result: two resident arrays are then 64 KB
// Interval<F64> items (gfti_series2_*): an LDS element is a 16-byte {lo, hi}, so two resident arrays are the same 64 KB at half that
constexpr unsigned SERIES2_MAX_ELEMS_IV = 2048;
constexpr unsigned SERIES3_MAX_ELEMS = 4096;  // n0 * n1 * n2 of the result: the two-arrays-in-64-KB footprint of rank 2
// Interval<F64> items (gfti_series3_*): 16-byte LDS elements, the same 64 KB at half that
constexpr unsigned SERIES3_MAX_ELEMS_IV = 2048;
// SERIES_OBSERVE_NEGBINOMIAL's own limit on 3 * degree_p1 + order: the lines D (degree_p1 + order elements), S and P (degree_p1 each)
// of its form B lie in the 64 KB of dynamic LDS every kernel may have (8-byte elements, 16-byte for Interval<F64>)
constexpr unsigned SERIES_NEGBIN_MAX = 8192;
constexpr unsigned SERIES_NEGBIN_MAX_IV = 4096;
// the most coefficients of an item's long side, by the rank (1, 2, 3) and the element width (1: F64, 2: Interval<F64>)
inline unsigned series_limit(int rank, int w) {
    constexpr unsigned most[3][2] = {{SERIES_MAX_N, SERIES_MAX_N_IV}, {SERIES2_MAX_ELEMS, SERIES2_MAX_ELEMS_IV}, {SERIES3_MAX_ELEMS, SERIES3_MAX_ELEMS_IV}};
    return most[rank - 1][w == 2];
}

// What the planes of a tensor hold.  SERIES_ELEM_BY_WIDTH, the default: the width alone says it -- w = 1 is F64, w = 2 is
// Interval<F64>, (lo, hi).  SERIES_ELEM_BIGFLOAT (w = 2): BigFloat (src/number/big_float.rs), the factor plane and the exponent plane
// (integral doubles); gftb_series_*, rank 1, the six arithmetic operations.
enum SeriesElem { SERIES_ELEM_BY_WIDTH = 0, SERIES_ELEM_BIGFLOAT = 1 };

// The element of a call: w = 1 is F64 (one plane, the strides below unused), w = 2 is Interval<F64>, stored as the planes
// (lo, hi) x / y / s / r elements apart (operands, seeds, result; 0 on an operand: a point interval read twice), or with
// elem == SERIES_ELEM_BIGFLOAT a BigFloat's (factor, exponent), where no plane stride is 0.
struct SeriesPlanes {
    int w = 1;
    size_t x = 0, y = 0, s = 0, r = 0;
    int elem = SERIES_ELEM_BY_WIDTH;
};

// The collapsed batch: item (i_0, ..., i_{nd-1}), row-major over ext, has its rows at x + sum i_a * xs[a] (elements), and
// likewise y (mul / div), the seeds (exp / log; one double per item) and the result.  Stride 0 repeats a row.
struct SeriesBatch {
    int nd = 0;
    unsigned items = 1;  // prod ext, < 2^31
    int inplace = 0;     // the result is one of the operands (the same view): a row is written by the workgroup that read it
    unsigned ext[IMAXD];
    size_t xs[IMAXD], ys[IMAXD], ss[IMAXD], rs[IMAXD];
};

// One item of an accepted call, at every rank: the stored shapes of x and y and the result's over the three series axes (slabs, rows,
// the unit-stride axis), right-aligned -- a lower rank has leading lengths of 1 -- and the element strides of those axes (0 under
// a length of 1, the last one 1).  exp / log / pow: ny is 1.
struct SeriesItem {
    unsigned nx[3], ny[3], n[3];
    size_t xs[3], ys[3], rs[3];
};
// the by-value parameter of the rank-2 kernels and of series_observe: the last two axes of an item
struct Series2Dims {
    unsigned nx0, nx1, ny0, ny1, n0, n1;  // stored shapes of x and y (exp / log / pow: ny* unused) and the result's; nx*, ny* <= n*
                                          // (SERIES_CORR / SERIES_COMPOSE_ADJ at rank 2: x is g / gh, the LONG side: ny*, n* <= nx*)
    size_t xr, yr, rr;                    // row strides in elements
};
static inline Series2Dims series2_dims(const SeriesItem& i) { return Series2Dims{i.nx[1], i.nx[2], i.ny[1], i.ny[2], i.n[1], i.n[2], i.xs[1], i.ys[1], i.rs[1]}; }

// One operand of a call as the C ABI states it: its lengths over the three series axes (slabs, rows, the unit-stride axis),
// right-aligned, and their strides in elements (st[2] is not read: that axis has unit stride).  A lower rank has leading lengths of
// 1 and strides of 0.  `bs`: nbatch batch strides in elements, for w == 2 preceded by the lo -> hi plane stride; null: contiguous
// items of the operand's own shape (the planes back to back).
struct SeriesView {
    const double* p = nullptr;
    const int64_t* bs = nullptr;
    size_t len[3] = {1, 1, 1};
    int64_t st[3] = {0, 0, 1};
};

// One call of rank 1, 2 or 3 (gft[i]_series_*, _series2_*, _series3_*): the limit bounds the product of the long side's lengths.
// What x, y and cs are to the op, which side is long and up to which rank the op exists: its row of SERIES_OPS.  Seeds and scalars
// are one double per item, so their lengths stay 1.  The transposed operations corr and compose_adj (whose result has nf
// coefficients) have the SHORT side as their result, so x bounds y and the result, and the rows the planner sizes are x's.
// `var`: compose's variable above rank 1, counted over the call's own axes (rank 3: 0 the slab axis, 1 the row axis, 2 the
// unit-stride axis).  The observation ops: `k` the order, `var` the axis at rank 2 (at rank 1 it is 1, the series axis), and the
// result's shape must be x's with k taken off that axis (evaluate_all_one: one element per item).  SERIES_OBSERVE_CHAIN: cs has
// len[2] = nsteps; the result has degree_p1 coefficients on the axis `var` and min(length, degree_p1) on the other one.
// SERIES_MUL_LINEAR / SERIES_COMPOSE_LINEAR: `var` (and compose_linear's `wvar`) the axes, at rank 1 both 1.
struct SeriesCall {
    int op = SERIES_MUL;
    const char* fn = "";  // the name in messages
    int w = 1;
    int elem = SERIES_ELEM_BY_WIDTH;  // what the w planes hold
    int rank = 1;
    uint32_t e = 0;
    int var = 0;
    int wvar = 0;  // compose_linear: the variable of the affine series (mul_linear: var is that variable)
    size_t k = 0;
    size_t nsteps = 0, degree_p1 = 0;
    const size_t* batch = nullptr;
    size_t nbatch = 0;
    SeriesView x, y, r, cs;
    SeriesView p;  // SERIES_OBSERVE_NEGBINOMIAL: the scalars p, one element per item as y
};

// What series_args makes of an accepted call: the collapsed batch, the plane strides and the item -- the lengths narrowed to
// unsigned (exact: the limits have been judged) with the strides of the series axes.
// `ps` / `pp`: the batch strides of SeriesCall::p over the collapsed axes and its plane stride (zeros where the op has no p).
struct SeriesArgs {
    SeriesBatch g;
    SeriesPlanes pl;
    SeriesItem it;
    size_t ps[IMAXD] = {};
    size_t pp = 0;
};

struct SeriesOperand {  // a view with its strides judged: batch strides in elements, the span it covers
    const char* what;
    const double* p;
    size_t len[3], ist[3];  // the series axes: a stride of 0 under a length of 1, the last one 1
    size_t st[32];
    size_t plane;  // w == 2: elements from the lo plane to the hi plane (0 on an operand: a point interval), else 0
    size_t span;   // elements from p to one past its last element (of the hi plane)
};

static inline SeriesOperand series_arg(const SeriesCall& c, const char* what, const SeriesView& v) {
    const std::string fn(c.fn);
    SeriesOperand a;
    a.what = what;
    a.p = v.p;
    a.len[2] = v.len[2], a.ist[2] = 1;
    a.span = v.len[2];
    for (int i = 1; i >= 0; --i) {
        if (v.st[i] < 0) throw std::runtime_error(fn + ": negative strides are not supported (" + what + (i ? ", the row axis)" : ", the slab axis)"));
        a.len[i] = v.len[i];
        a.ist[i] = v.len[i] > 1 ? (size_t)v.st[i] : 0;
        a.span += (v.len[i] - 1) * a.ist[i];
    }
    size_t cs = v.len[2] * v.len[1] * v.len[0];  // NULL: contiguous items of the operand's own shape (the planes back to back)
    const int64_t* bs = v.bs;
    if (c.w == 2 && bs) {
        if (bs[0] < 0) throw std::runtime_error(fn + ": negative strides are not supported (" + what + ", the plane axis)");
        ++bs;
    }
    for (size_t i = c.nbatch; i-- > 0;) {
        if (bs && bs[i] < 0)
            throw std::runtime_error(fn + ": negative strides are not supported (" + what + ", batch axis " + std::to_string(i) + ")");
        a.st[i] = bs ? (size_t)bs[i] : cs;
        cs *= c.batch[i];
        a.span += (c.batch[i] - 1) * a.st[i];
    }
    a.plane = c.w == 2 ? (bs ? (size_t)bs[-1] : cs) : 0;
    a.span += a.plane;
    return a;
}

static inline bool series_same_view(const SeriesOperand& a, const SeriesOperand& b, const size_t* batch, size_t nbatch) {
    if (a.p != b.p || a.plane != b.plane) return false;
    for (int i = 0; i < 3; ++i)
        if (a.len[i] != b.len[i] || a.ist[i] != b.ist[i]) return false;
    for (size_t i = 0; i < nbatch; ++i)
        if (batch[i] > 1 && a.st[i] != b.st[i]) return false;
    return true;
}

// The shape rules of the affine substitutions (ranks 1 and 2; at rank 1 var == wvar == 1, the series axis): the axes, a result of at
// least two coefficients on the affine series' axis, an operand inside the result, the limit on the result.
static inline void series_linear_shapes(const SeriesCall& c) {
    using std::to_string;
    const std::string f(c.fn);
    const bool r2 = c.rank > 1, comp = c.op == SERIES_COMPOSE_LINEAR;
    const char* const who = series_op_row(c.op).x;
    if (r2 && (c.var < 0 || c.var > 1))
        throw std::runtime_error(f + ": var = " + to_string(c.var) + (comp ? " (the variable of f that is replaced is 0 or 1)" : " (the variable of the linear factor is 0 or 1)"));
    if (r2 && comp && (c.wvar < 0 || c.wvar > 1))
        throw std::runtime_error(f + ": wvar = " + to_string(c.wvar) + " (the variable of the affine series is 0 or 1)");
    const int w = comp ? c.wvar : c.var;
    if (c.r.len[1] == 0 || c.r.len[2] == 0)
        throw std::runtime_error(f + (r2 ? ": n0 * n1 == 0 (the result has no coefficients)" : ": n == 0 (the result has no coefficients)"));
    const size_t nw = c.r.len[1 + w];
    if (nw < 2)
        throw std::runtime_error(f + ": the result has " + to_string(nw) + " coefficient" + (r2 ? " on axis " + to_string(w - 2) : std::string()) +
                                 " (c + m * x needs two: a substitution at one coefficient is the constant one, not a linear one)");
    if (c.x.len[1] == 0 || c.x.len[2] == 0) throw std::runtime_error(f + ": an operand has no coefficients");
    if (c.x.len[1] > c.r.len[1] || c.x.len[2] > c.r.len[2]) {
        if (r2)
            throw std::runtime_error(f + ": " + who + " has " + to_string(c.x.len[1]) + " x " + to_string(c.x.len[2]) + " coefficients, the result " +
                                     to_string(c.r.len[1]) + " x " + to_string(c.r.len[2]) + " (an operand is longer than the truncation order)");
        throw std::runtime_error(f + ": n" + who + " = " + to_string(c.x.len[2]) + " > n = " + to_string(c.r.len[2]) + " (an operand is longer than the truncation order)");
    }
    const size_t most = series_limit(c.rank, c.w);
    if (c.r.len[1] > most || c.r.len[2] > most || c.r.len[1] * c.r.len[2] > most) {
        if (r2)
            throw std::runtime_error(f + ": n0 * n1 = " + to_string(c.r.len[1]) + " * " + to_string(c.r.len[2]) + " exceeds the limit of " + to_string(most) +
                                     " coefficients per item of this version");
        throw std::runtime_error(f + ": n = " + to_string(c.r.len[2]) + " exceeds the limit of " + to_string(most) + " coefficients per series of this version");
    }
}

// The three shape rules, once over the call's `rank` series axes: nothing is empty, the long side carries the limit, and the short
// sides fit inside the long side.  The long side is the result, or x for the transposed and the observation ops (ranks 1 and 2).
// The texts are per rank: rank 1 names its lengths, the higher ranks print the last `rank` lengths of a view.
// (static, as everything below: the library exports none of this layer)
static inline void series_shapes(const SeriesCall& c) {
    using std::to_string;
    const std::string f(c.fn);
    const SeriesOpRow& row = series_op_row(c.op);
    const int op = c.op, rank = c.rank;
    if (c.elem == SERIES_ELEM_BIGFLOAT) {  // the BigFloat family: rank 1, the six arithmetic operations, two planes
        if (rank != 1) throw std::runtime_error(f + ": BigFloat series exist at rank 1 only in this version (rank " + to_string(rank) + " was asked for)");
        if (op > SERIES_POW) throw std::runtime_error(f + ": no such operation on BigFloat series in this version (mul / div / exp / log / compose / pow)");
        if (c.w != 2) throw std::runtime_error(f + ": a BigFloat tensor has two planes (factor, exponent), not " + to_string(c.w));
    }
    // (the text is pinned byte for byte by tests/series3_compose_args_main.cpp and tests/series_refusals.json; its "on f64" dates from
    // before gfti_series3_* and misleads an interval caller or one with another width -- to be retired with those pins)
    if (rank == 3 && ((c.w != 1 && c.w != 2) || row.ranks < 3))
        throw std::runtime_error(f + ": no such operation at rank 3 in this version (mul / div / exp / log on f64)");
    if (row.family == SERIES_LINEAR) return series_linear_shapes(c);
    if (op == SERIES_LAH_ROW) {  // the one rule: order + 1 entries within the rank-1 limit (the operand is one scalar per item)
        const size_t most = series_limit(1, c.w);
        if (c.r.len[2] == 0 || c.r.len[2] > most)
            throw std::runtime_error(f + ": order + 1 = " + (c.r.len[2] ? to_string(c.r.len[2]) : std::string("2^64")) + " exceeds the limit of " + to_string(most) +
                                     " coefficients per series of this version");
        return;
    }
    const bool negbin = op == SERIES_OBSERVE_NEGBINOMIAL;
    const bool chain = row.family == SERIES_CHAIN, observe = chain || row.family == SERIES_OBSERVE;
    const bool corr = op == SERIES_CORR, adj = op == SERIES_COMPOSE_ADJ, binary = row.yrole == SERIES_Y_SERIES, xlong = row.xlong;
    const bool r2 = rank > 1, bad_var = r2 && (c.var < 0 || c.var >= rank);
    if (bad_var && (op == SERIES_COMPOSE || adj))
        throw std::runtime_error(f + ": var = " + to_string(c.var) + " (the variable of f that g replaces is " + (rank == 3 ? "0, 1 or 2)" : "0 or 1)"));
    struct Names {
        std::string x, y, r;
    };
    // the row's names -- but compose, f / g everywhere else, is x / y in these texts below rank 3 (pinned as found)
    const bool xy = op == SERIES_COMPOSE && rank < 3;
    const Names who{xy ? "x" : row.x, xy ? "y" : row.y, "the result"};
    // rank 1 names its lengths: n and the operand's name, the result's n; corr's result has m, compose_adj's gh has n and its result nf
    const Names len{adj ? "n" : "n" + who.x, "n" + who.y, corr ? "m" : (adj ? "nf" : "n")};
    const char* const shape = rank == 3 ? "n0 * n1 * n2" : "n0 * n1";  // above rank 1: the result's lengths by name
    const SeriesView& L = xlong ? c.x : c.r;
    const std::string &Llen = xlong ? len.x : len.r, &Lwho = xlong ? who.x : who.r;
    auto empty = [](const SeriesView& v) { return v.len[0] == 0 || v.len[1] == 0 || v.len[2] == 0; };
    auto dims = [rank](const SeriesView& v, const char* sep) {  // the last `rank` lengths
        std::string t = to_string(v.len[2]);
        for (int i = 1; i >= 3 - rank; --i) t = to_string(v.len[i]) + sep + t;
        return t;
    };
    if (observe) {
        if (empty(c.x)) throw std::runtime_error(f + ": " + who.x + " has no coefficients");
    } else if (empty(c.r)) {
        if (!r2) throw std::runtime_error(f + ": " + len.r + " == 0 (the result has no coefficients)");
        throw std::runtime_error(f + (xlong ? ": the result has no coefficients (an axis of its shape is 0)" : std::string(": ") + shape + " == 0 (the result has no coefficients)"));
    }
    const size_t most = series_limit(rank, c.w);
    bool over = false;  // a length or a partial product of the lengths (none overflows: every factor is within the limit)
    for (size_t i = 0, prod = 1; i < 3 && !over; ++i) over = L.len[i] > most || (prod *= L.len[i]) > most;
    if (over) {
        if (!r2)
            throw std::runtime_error(f + ": " + Llen + " = " + to_string(L.len[2]) + " exceeds the limit of " + to_string(most) + " coefficients per series of this version");
        if (xlong)
            throw std::runtime_error(f + ": " + Lwho + " has " + dims(L, " * ") + " coefficients, which exceeds the limit of " + to_string(most) +
                                     " coefficients per item of this version");
        throw std::runtime_error(f + ": " + shape + " = " + dims(L, " * ") + " exceeds the limit of " + to_string(most) + " coefficients per item of this version");
    }
    if (observe) {
        if (bad_var) throw std::runtime_error(f + ": var = " + to_string(c.var) + " (the variable the operation acts on is 0 or 1)");
        if (op == SERIES_EVAL_ONE) return;
        const bool rows = r2 && c.var == 0;
        if (chain) {  // degree_p1 + nsteps <= L_0: step t then runs at d_t = degree_p1 + (nsteps - 1 - t) on a line of d_t + 1
            const size_t L0 = rows ? c.x.len[1] : c.x.len[2], other = rows ? c.x.len[2] : c.x.len[1], d = c.degree_p1;
            const std::string on = r2 ? " on axis " + to_string(c.var) : std::string();
            if (negbin) {  // order = K: pass i reads d coefficients of the i-th derivative, so degree_p1 + K <= L_0; the powers need d >= 3
                const size_t n = c.cs.len[2], own = c.w == 2 ? SERIES_NEGBIN_MAX_IV : SERIES_NEGBIN_MAX;
                if (n == 0) throw std::runtime_error(f + ": ls holds no entry (a row of order K has K + 1 >= 1 entries)");
                if (d < 3)
                    throw std::runtime_error(f + ": degree_p1 = " + to_string(d) + " (the result needs at least three coefficients" + on +
                                             ": degree_p1 >= 3; at two the reference multiplies by a linear power in every pass, a form this version leaves out)");
                if (d > L0 || n - 1 > L0 - d)
                    throw std::runtime_error(f + ": degree_p1 + order = " + to_string(d) + " + " + to_string(n - 1) + ", but a has " + to_string(L0) +
                                             " stored coefficients" + on + " (every pass takes one: degree_p1 + order <= " + to_string(L0) + ")");
                if (3 * d + (n - 1) > own)
                    throw std::runtime_error(f + ": 3 * degree_p1 + order = 3 * " + to_string(d) + " + " + to_string(n - 1) + " exceeds the limit of " + to_string(own) +
                                             " of this operation (three lines of a pass lie in 64 KB of LDS)");
                const size_t o = std::min(other, d), w0 = rows ? d : o, w1 = rows ? o : d;
                if (c.r.len[1] != (r2 ? w0 : 1) || c.r.len[2] != w1)
                    throw std::runtime_error(f + ": the result has " + (r2 ? to_string(c.r.len[1]) + " x " : std::string()) + to_string(c.r.len[2]) +
                                             " coefficients; with degree_p1 = " + to_string(d) + " it has " + (r2 ? to_string(w0) + " x " : std::string()) + to_string(w1));
                return;
            }
            if (c.nsteps == 0) throw std::runtime_error(f + ": nsteps = 0 (cs holds no constants: a chain has at least one step)");
            if (d < 2) throw std::runtime_error(f + ": degree_p1 = " + to_string(d) + " (the result needs at least two coefficients" + on + ": degree_p1 >= 2)");
            if (d > L0 || c.nsteps > L0 - d)
                throw std::runtime_error(f + ": degree_p1 + nsteps = " + to_string(d) + " + " + to_string(c.nsteps) + ", but a has " + to_string(L0) +
                                         " stored coefficients" + on + " (every step takes one: degree_p1 + nsteps <= " + to_string(L0) + ")");
            const size_t o = std::min(other, d), w0 = rows ? d : o, w1 = rows ? o : d;
            if (c.r.len[1] != (r2 ? w0 : 1) || c.r.len[2] != w1)
                throw std::runtime_error(f + ": the result has " + (r2 ? to_string(c.r.len[1]) + " x " : std::string()) + to_string(c.r.len[2]) +
                                         " coefficients; with degree_p1 = " + to_string(d) + " it has " + (r2 ? to_string(w0) + " x " : std::string()) + to_string(w1));
            return;
        }
        const size_t n = rows ? c.x.len[1] : c.x.len[2], k = c.k;
        if (k >= n)
            throw std::runtime_error(f + ": k = " + to_string(k) + ", but x has " + to_string(n) + " stored coefficients" +
                                     (r2 ? " on axis " + to_string(c.var) : std::string()) + " (the order must satisfy 0 <= k < " + to_string(n) + ")");
        const size_t w0 = rows ? c.x.len[1] - k : c.x.len[1], w1 = rows ? c.x.len[2] : c.x.len[2] - k;
        if (c.r.len[1] != w0 || c.r.len[2] != w1)
            throw std::runtime_error(f + ": the result has " + (r2 ? to_string(c.r.len[1]) + " x " : std::string()) + to_string(c.r.len[2]) + " coefficients; with k = " +
                                     to_string(k) + " it has " + (r2 ? to_string(w0) + " x " : std::string()) + to_string(w1) + " (x's, less k on the axis)");
        return;
    }
    if (empty(c.x) || (binary && empty(c.y))) throw std::runtime_error(f + ": an operand has no coefficients");
    auto fits = [&](const SeriesView& s, const std::string& slen, const std::string& swho) {
        if (s.len[0] <= L.len[0] && s.len[1] <= L.len[1] && s.len[2] <= L.len[2]) return;
        const char* why = &s == &c.r ? "the result of a transposed operation is its short side" : "an operand is longer than the truncation order";
        if (r2) throw std::runtime_error(f + ": " + swho + " has " + dims(s, " x ") + " coefficients, " + Lwho + " " + dims(L, " x ") + " (" + why + ")");
        throw std::runtime_error(f + ": " + slen + " = " + to_string(s.len[2]) + " > " + Llen + " = " + to_string(L.len[2]) + " (" + why + ")");
    };
    if (xlong) fits(c.r, len.r, who.r);  // (the transposed ops: the observation ops have returned)
    else fits(c.x, len.x, who.x);
    if (binary) fits(c.y, len.y, who.y);
}

// Judges one call and plans its batch.  The order of the checks: the shapes; nbatch and a null batch; an empty batch (returns
// false: nothing to do, no stride is looked at); 2^31 items; negative strides; zero or overlapping result strides; check_ptr(p,
// what) on x, y and the result (the one step that needs the device: the caller's); the overlap proof; the collapse.  Throws
// std::runtime_error with the message of the refusal.
template <class CheckPtr>
static inline bool series_args(const SeriesCall& c, SeriesArgs& out, CheckPtr&& check_ptr) {
    const std::string f(c.fn);
    const SeriesOpRow& row = series_op_row(c.op);
    const int w = c.w;
    const size_t* batch = c.batch;
    const size_t nbatch = c.nbatch;
    series_shapes(c);
    if (nbatch > 32) throw std::runtime_error(f + ": more than 32 batch axes");
    if (nbatch && !batch) throw std::runtime_error(f + ": the batch shape is a null pointer");
    size_t items = 1;
    for (size_t i = 0; i < nbatch; ++i) {
        if (batch[i] == 0) return false;  // an empty batch: nothing to do
        items *= batch[i];
        if (items >= ((size_t)1 << 31)) throw std::runtime_error(f + ": more than 2^31 - 1 series in one call");
    }
    const SeriesOperand ax = series_arg(c, row.x, c.x);
    const SeriesOperand ay = series_arg(c, row.y, c.y);
    const SeriesOperand ar = series_arg(c, "the result", c.r);
    const SeriesOperand ac = series_arg(c, row.cs, c.cs);
    const bool has_p = c.op == SERIES_OBSERVE_NEGBINOMIAL;
    const SeriesOperand ap = series_arg(c, "p", c.p);  // (the default view where the op has none: nothing about it can be refused)
    // y is read where the op has one and, where it is optional (the seeds, the chain's x), it is given; cs where the op has one
    const bool optional = row.yrole == SERIES_Y_SEEDS || (row.family == SERIES_CHAIN && !has_p);
    const bool has_y = row.yrole != SERIES_Y_NONE && (ay.p || !optional), has_cs = row.csrole != SERIES_CS_NONE;
    if (c.elem == SERIES_ELEM_BIGFLOAT) {  // a point interval reads one plane twice; a factor plane cannot be its own exponent plane
        const SeriesOperand* const read[2] = {&ax, has_y ? &ay : nullptr};  // (the result's is refused below, for intervals too)
        for (const SeriesOperand* a : read)
            if (a && a->plane == 0)
                throw std::runtime_error(f + ": zero plane stride on " + a->what + " (the factor plane of a BigFloat tensor cannot be its own exponent plane)");
    }
    // the result's elements are distinct addresses: no zero stride, and sorted by stride every axis steps over the ones below it
    {
        struct Ax {
            size_t ext, st;
        } axes[36];
        int k = 0;
        if (w == 2) {  // the two planes are one more axis of the result
            if (ar.plane == 0) throw std::runtime_error(f + ": the result has a zero plane stride: its lower and upper bounds overlap");
            axes[k++] = Ax{2, ar.plane};
        }
        for (size_t i = 0; i < nbatch; ++i) {
            if (batch[i] <= 1) continue;
            if (ar.st[i] == 0) throw std::runtime_error(f + ": the result has a zero stride (batch axis " + std::to_string(i) + "): its series overlap");
            axes[k++] = Ax{batch[i], ar.st[i]};
        }
        if (ar.len[1] > 1) {  // rank 2: the rows of an item are one more axis of the result
            if (ar.ist[1] == 0) throw std::runtime_error(f + ": the result has a zero row stride: the rows of an item overlap");
            axes[k++] = Ax{ar.len[1], ar.ist[1]};
        }
        if (ar.len[0] > 1) {  // rank 3: the slabs of an item are one more axis again
            if (ar.ist[0] == 0) throw std::runtime_error(f + ": the result has a zero slab stride: the slabs of an item overlap");
            axes[k++] = Ax{ar.len[0], ar.ist[0]};
        }
        if (ar.len[2] > 1) axes[k++] = Ax{ar.len[2], 1};
        std::sort(axes, axes + k, [](const Ax& u, const Ax& v) { return u.st < v.st; });
        for (int i = 1; i < k; ++i)
            if (axes[i].st / axes[i - 1].ext < axes[i - 1].st)
                throw std::runtime_error(f + ": the result's series overlap each other (its strides do not separate the rows)");
    }
    check_ptr(ax.p, ax.what);
    if (has_y) check_ptr(ay.p, ay.what);
    if (has_cs) check_ptr(ac.p, ac.what);
    if (has_p) check_ptr(ap.p, ap.what);
    check_ptr(ar.p, ar.what);
    // the result may be an input itself (the same view: every row is read before it is written); any other overlap is refused.
    // Judged by address ranges, so two interleaved views of one buffer count as overlapping.
    bool inplace = false;
    auto overlap = [&](const SeriesOperand& a, bool same_ok) {
        if (a.p + a.span <= ar.p || ar.p + ar.span <= a.p) return;
        if (same_ok && series_same_view(a, ar, batch, nbatch)) {
            inplace = true;
            return;
        }
        throw std::runtime_error(f + ": the result partially overlaps " + a.what + " (it may alias an operand only as the same view)");
    };
    overlap(ax, row.alias_x);
    if (has_cs) overlap(ac, false);
    if (has_y) overlap(ay, row.alias_y);
    if (has_p) overlap(ap, false);
    // collapse the batch: unit axes go, axes contiguous with their inner neighbour on every operand merge
    SeriesBatch& g = out.g;
    g.nd = 0;
    g.items = (unsigned)items;
    g.inplace = inplace;
    // what travels as ys / pl.y and as ss / pl.s: a second series or a scalar y as y; the seeds, else cs, as s
    const SeriesOperand* const as_y = has_y && row.yrole != SERIES_Y_SEEDS ? &ay : nullptr;
    const SeriesOperand* const as_s = has_y && row.yrole == SERIES_Y_SEEDS ? &ay : (has_cs ? &ac : nullptr);
    for (size_t i = 0; i < nbatch; ++i) {
        if (batch[i] == 1) continue;
        const size_t e = batch[i], sx = ax.st[i], sy = as_y ? as_y->st[i] : 0, ss = as_s ? as_s->st[i] : 0, sr = ar.st[i];
        const size_t sp = has_p ? ap.st[i] : 0;
        int p = g.nd - 1;
        // (merged extents stay below 2^31: items does)
        if (p >= 0 && g.xs[p] == sx * e && g.ys[p] == sy * e && g.ss[p] == ss * e && g.rs[p] == sr * e && out.ps[p] == sp * e) {
            g.ext[p] *= (unsigned)e;
        } else {
            // (the workspace copies add the series axis, and for intervals the plane axis, to these; pow's copy every series axis of the rank)
            const int most = IMAXD - w - (row.family == SERIES_POWER ? c.rank - 1 : 0);
            if (g.nd == most) throw std::runtime_error(f + ": the batch has more than " + std::to_string(most) + " non-contiguous axes");
            p = g.nd++;
            g.ext[p] = (unsigned)e;
        }
        g.xs[p] = sx, g.ys[p] = sy, g.ss[p] = ss, g.rs[p] = sr, out.ps[p] = sp;
    }
    out.pp = has_p ? ap.plane : 0;
    out.pl.w = w;
    out.pl.elem = c.elem;
    out.pl.x = ax.plane;
    out.pl.y = as_y ? as_y->plane : 0;
    out.pl.s = as_s ? as_s->plane : 0;
    out.pl.r = ar.plane;
    SeriesItem& it = out.it;
    for (int i = 0; i < 3; ++i) {
        it.nx[i] = (unsigned)ax.len[i], it.ny[i] = (unsigned)ay.len[i], it.n[i] = (unsigned)ar.len[i];
        it.xs[i] = ax.ist[i], it.ys[i] = ay.ist[i], it.rs[i] = ar.ist[i];
    }
    return true;
}

// ---- rank 3: what is computed, decided by the shapes alone -----------------------------------------------------------------------
// An item in the order the kernels run it.  The reference computes on the stored result shape S, not on n (S_a per axis: mul
// min(n_a, nx_a + ny_a - 1), sum_shape mt:150-170; div n_a, but nx_a where ny_a == 1, mt:1216-1221; exp / log n_a, but 1 where
// nx_a == 1, mt:408-413), and an S with a unit axis is by definition the item WITHOUT that axis: the rank-2 item, the series row,
// the scalar.  So the axes are permuted: the unit axes of S go to the front and the others keep their order behind them --
// S = (5, 3, 1) runs as (1, 5, 3), the innermost axis then striding by the row stride.  With a leading unit axis the rank-3 loops
// ARE the rank-2 loops (one slab, whose step is the rank-2 body), with two the rank-1 loops.  Everything of n outside S is +0.0.
struct Series3Dims {
    unsigned nx[3], ny[3], n[3];  // permuted: the stored shapes of x and y (exp / log: ny unused) and S
    size_t xs[3], ys[3], rs[3];   // permuted: the element strides of the three axes of x, y and the result
    unsigned full[3], keep[3];    // as the caller states them: n and S, for the zero fill
    size_t fs[3];                 // and the result's strides
};
// (on the shapes and element strides in the caller's axis order)
static inline Series3Dims series3_dims(int op, const unsigned* nx, const unsigned* ny, const unsigned* n, const size_t* xs, const size_t* ys,
                                       const size_t* rs) {
    Series3Dims k;
    int order[3], m = 0;
    for (int i = 0; i < 3; ++i) {
        unsigned s = n[i];
        if (op == SERIES_MUL) s = std::min(n[i], nx[i] + ny[i] - 1);
        else if (op == SERIES_DIV) s = ny[i] == 1 ? nx[i] : n[i];
        else if (nx[i] == 1) s = 1;
        k.full[i] = n[i], k.keep[i] = s, k.fs[i] = rs[i];
    }
    for (int i = 0; i < 3; ++i)
        if (k.keep[i] == 1) order[m++] = i;
    for (int i = 0; i < 3; ++i)
        if (k.keep[i] != 1) order[m++] = i;
    const bool binary = op == SERIES_MUL || op == SERIES_DIV;
    for (int i = 0; i < 3; ++i) {
        const int o = order[i];
        // (an operand axis under a unit axis of S has one coefficient: it is no longer than S)
        k.nx[i] = nx[o], k.ny[i] = binary ? ny[o] : 1, k.n[i] = k.keep[o];
        k.xs[i] = xs[o], k.ys[i] = binary ? ys[o] : 0, k.rs[i] = rs[o];
    }
    return k;
}
static inline Series3Dims series3_dims(int op, const SeriesItem& i) { return series3_dims(op, i.nx, i.ny, i.n, i.xs, i.ys, i.rs); }

// The scratch of div / exp / log at rank 3 (gft_series3.hip's planner, here without the device): behind the resident operand and the
// result, `selems` elements (w * 8 bytes each) of row sums out of `budget` bytes of LDS, and the terms per chunk `tc`.  An item of one
// slab is the rank-2 item: rows of n2 elements, one at least where a row has terms; else chunks of whole slabs of n1 * n2, one at
// least.  `need`: the smallest scratch, `want`: the one that takes every term at once; `fits`: resident + need lie within the budget.
struct Series3Sizes {
    size_t resident = 0, need = 0, want = 0;  // elements
    unsigned selems = 0, tc = 0;
    bool fits = true;
};
static inline Series3Sizes series3_sizes(int op, const Series3Dims& d, int w, size_t budget) {
    Series3Sizes z;
    const size_t elem = (size_t)w * sizeof(double);
    const unsigned n12 = d.n[1] * d.n[2], N = d.n[0] * n12;
    const unsigned* a = op == SERIES_DIV ? d.ny : d.nx;
    z.resident = (size_t)a[0] * a[1] * a[2] + N;
    const unsigned terms0 = std::min(d.n[0], a[0]) - 1, J1 = std::min(d.n[1], a[1]);  // of the longest j0 range; places of j1
    const unsigned terms2 = J1 - 1;                                            // of the longest j range of a rank-2 row
    if (d.n[0] == 1) z.need = terms2 ? d.n[2] : 0, z.want = (size_t)terms2 * d.n[2];
    else z.need = n12, z.want = std::max<size_t>((size_t)terms0 * J1, 1) * n12;
    if (z.need) {
        z.fits = (z.resident + z.need) * elem <= budget;
        if (z.fits) z.selems = (unsigned)std::min(z.want, budget / elem - z.resident);
    }
    z.tc = d.n[0] == 1 ? 0 : (unsigned)std::min<size_t>((size_t)terms0 * J1, z.selems / n12);
    return z;
}

// mul3(a, b, L), the one product compose and pow are made of: series3.mul on two COMPACT (row-major) items of the stored shapes a
// and b, truncated at L.  The result is compact at L too, or lies at the element strides `rs` (pow's last product, which writes the
// caller's result).  Both of mul's rules apply through series3_dims: computed on S = min(L, a + b - 1), the unit axes of S in front.
static inline Series3Dims series3_product_dims(const unsigned* a, const unsigned* b, const unsigned* L, const size_t* rs = nullptr) {
    const size_t as[3] = {(size_t)a[1] * a[2], a[2], 1}, bs[3] = {(size_t)b[1] * b[2], b[2], 1}, ls[3] = {(size_t)L[1] * L[2], L[2], 1};
    return series3_dims(SERIES_MUL, a, b, L, as, bs, rs ? rs : ls);
}
// the compact shape of a product in compose's and pow's chains: min(a + b - 1, n) per axis (sum_shape)
static inline void series3_compact(const unsigned* a, const unsigned* b, const unsigned* n, unsigned* L) {
    for (int i = 0; i < 3; ++i) L[i] = std::min(a[i] + b[i] - 1, n[i]);
}

// ---- rank 3: compose (subst_var's Horner path) ---------------------------------------------------------------------------------------
// res = 0.0 + the last slice of f along axis `var` (stored shape: nf with 1 on that axis); for every earlier slice, last to first:
// res = mul3(res, g, L) at L = series3_compact(res, g, n), then the slice is added into res[index 0 on axis var].  Every product is
// series3.mul's, so it runs on the permuted item of ITS stored shape L -- and that permutation is the same for every step of a call:
// L_a == 1 iff n_a == 1, or ng_a == 1 and res started with 1 on the axis (a == var, or nf_a == 1); an axis that starts longer, or that
// g lengthens, has L_a >= 2 from the first step on and only grows.  So the unit axes of every step are those of the final stored shape
// S, one permutation (the unit axes of S in front, as in series3_dims) serves the whole loop, and the kernel runs the chain on the
// permuted item.  series3_compose_dims walks the steps and throws std::logic_error should a step ever disagree.
struct Series3Compose {
    unsigned sl[3], ng[3], n[3];  // permuted: a slice of f (nf with 1 on var's axis: where res starts), g's stored shape, the orders n
    unsigned s[3];                // permuted: the final stored shape S of res
    size_t xs[3], ys[3], rs[3];   // permuted: the element strides of f, g and the result
    unsigned slices;              // of f along var, `fslice` elements apart
    size_t fslice;
    int var;                      // the permuted position of var
    unsigned full[3], keep[3];    // as the caller states them: n and S, for the zero fill
    size_t fs[3];                 // and the result's strides
};
static inline Series3Compose series3_compose_dims(const unsigned* nf, const unsigned* ng, const unsigned* n, const size_t* xs, const size_t* ys,
                                                  const size_t* rs, int var) {
    if (var < 0 || var > 2) throw std::logic_error("series3_compose_dims: var outside 0 .. 2");
    Series3Compose k;
    unsigned r[3] = {nf[0], nf[1], nf[2]}, L[3];
    r[var] = 1;
    const unsigned steps = nf[var] - 1;
    // the final stored shape: every axis is non-decreasing and settles after at most n_a steps
    unsigned S[3] = {r[0], r[1], r[2]};
    for (unsigned i = 0; i < steps; ++i) {
        series3_compact(S, ng, n, L);
        if (L[0] == S[0] && L[1] == S[1] && L[2] == S[2]) break;
        S[0] = L[0], S[1] = L[1], S[2] = L[2];
    }
    // the invariance of the unit axes over the steps (above)
    for (unsigned i = 0; i < steps; ++i) {
        series3_compact(r, ng, n, L);
        for (int a = 0; a < 3; ++a)
            if ((L[a] == 1) != (S[a] == 1)) throw std::logic_error("series3_compose_dims: the unit axes of a step differ from those of the final shape");
        if (L[0] == r[0] && L[1] == r[1] && L[2] == r[2]) break;
        r[0] = L[0], r[1] = L[1], r[2] = L[2];
    }
    int order[3], m = 0;
    for (int i = 0; i < 3; ++i) k.full[i] = n[i], k.keep[i] = S[i], k.fs[i] = rs[i];
    for (int i = 0; i < 3; ++i)
        if (S[i] == 1) order[m++] = i;
    for (int i = 0; i < 3; ++i)
        if (S[i] != 1) order[m++] = i;
    k.var = 0;
    for (int i = 0; i < 3; ++i) {
        const int o = order[i];
        if (o == var) k.var = i;
        k.sl[i] = o == var ? 1 : nf[o], k.ng[i] = ng[o], k.n[i] = n[o], k.s[i] = S[o];
        k.xs[i] = xs[o], k.ys[i] = ys[o], k.rs[i] = rs[o];
    }
    k.slices = nf[var], k.fslice = xs[var];
    return k;
}
static inline Series3Compose series3_compose_dims(const SeriesItem& i, int var) { return series3_compose_dims(i.nx, i.ny, i.n, i.xs, i.ys, i.rs, var); }

// ---- pow at every rank: the products of the square-and-multiply loop (mt:441-450), decided by e and the shapes alone ------------------
// res = [1.0]; while e > 0: if e is odd, res = res * base; e >>= 1; if e > 0, base = base * base -- every product at the compact
// shape series3_compact(a, b, n).  The operands live in slots: the unit item, three workspace arrays (x is copied into the first,
// the other two take turns as outputs, and an array is free again once its item has been multiplied away) and the caller's result,
// which the last product writes at all of n.  An output slot is never one of its operands'.
enum SeriesPowSlot { POW_UNIT = 0, POW_WS0 = 1, POW_WS1 = 2, POW_WS2 = 3, POW_RESULT = 4 };
struct SeriesPowStep {
    int a, b, out;               // slots: out = a * b (accumulator times base, or base times base)
    unsigned sa[3], sb[3], L[3];  // the stored shapes of a and b, and the compact shape of the product
    bool last;
};
struct SeriesPowSteps {
    int count = 0;  // popcount(e) + floor(log2 e): at most 63 of a 32-bit e, none of e == 0
    SeriesPowStep step[63];
};
// (nx: the stored shape of x, n: the orders; three right-aligned lengths each)
static inline SeriesPowSteps series_pow_steps(uint32_t e, const unsigned* nx, const unsigned* n) {
    SeriesPowSteps p;
    int acc = POW_UNIT, base = POW_WS0, spare[2] = {POW_WS1, POW_WS2}, nspare = 2;
    unsigned la[3] = {1, 1, 1}, lb[3] = {nx[0], nx[1], nx[2]};
    auto product = [&](int a, const unsigned* sa, int b, const unsigned* sb, bool last) -> SeriesPowStep& {
        SeriesPowStep& s = p.step[p.count++];
        s.a = a, s.b = b, s.out = last ? (int)POW_RESULT : spare[--nspare], s.last = last;
        for (int i = 0; i < 3; ++i) s.sa[i] = sa[i], s.sb[i] = sb[i];
        series3_compact(sa, sb, n, s.L);
        return s;
    };
    while (e > 0) {
        if (e & 1) {
            const SeriesPowStep& s = product(acc, la, base, lb, (e >> 1) == 0);
            if (acc != POW_UNIT) spare[nspare++] = acc;
            acc = s.out;
            for (int i = 0; i < 3; ++i) la[i] = s.L[i];
        }
        e >>= 1;
        if (e > 0) {
            const SeriesPowStep& s = product(base, lb, base, lb, false);
            spare[nspare++] = base;
            base = s.out;
            for (int i = 0; i < 3; ++i) lb[i] = s.L[i];
        }
    }
    return p;
}

}  // namespace gft
