// ------------------------------------------------------------------------------------------
// batched univariate series on caller-owned device tensors: gft_series_mul / div / exp / log / compose / pow / corr / compose_adj,
// and the first six's Interval<F64> twins gfti_series_* (w == 2: every stride array starts with the lo -> hi plane stride)
// and the bivariate gft_series2_mul / div / exp / log / compose / pow with their Interval<F64> twins gfti_series2_* (the same
// validation with one row stride per operand), and the f64-only transposed gft_series2_corr / compose_adj
// and the trivariate gft_series3_mul / div / exp / log / compose / pow with their Interval<F64> twins gfti_series3_* (a slab stride and a row stride per operand; computed
// at the stored result shape S on the permuted item of gft::series3_dims, compose on that of gft::series3_compose_dims)
// and the observation ops gft_series_* / gft_series2_* derivative / taylor_expansion_of_coeff / shift_down / evaluate_all_one with
// their gfti_ twins (one operand, the result shorter by the order k on one axis; the kernels: gft_series_observe.hip)
// and the fused observation chain gft_series_observe_chain / gft_series2_observe_chain with their gfti_ twins (every item with its
// own scalars x and constants cs, one launch for all the steps; the kernels: gft_series_observe_chain.hip)
// and the affine substitutions gft_series_mul_linear / compose_linear, gft_series2_mul_linear / compose_linear with their gfti_ twins
// (every item with its own scalars c and m, one launch; the kernels: gft_series_linear.hip)
// and the fused negative-binomial observation gft_series_observe_negbinomial / gft_series2_observe_negbinomial with the Lah row
// gft_series_lah_row and their gfti_ twins (every item with its own scalars x and p and its own row; the kernels:
// gft_series_observe_negbinomial.hip)
// and the BigFloat family gftb_series_mul / div / exp / log / compose / pow (rank 1 only; w == 2 with the element kind
// gft::SERIES_ELEM_BIGFLOAT: every stride array starts with the factor -> exponent plane stride)
// Every entry point fills one gft::SeriesCall with its rank (gft_series_args.hpp, which judges it without the device and states the
// item of any rank as one gft::SeriesItem) and hands it to series_call, which dispatches on the family of the op's row in
// gft::SERIES_OPS and, for the arithmetic family, on the rank; pow is one driver.
// (the planner and the kernels: gft_series.hpp, gft_series.hip; included by gft_api.hip after the device interop, whose
// pointer check and stream joins it shares)
// ------------------------------------------------------------------------------------------
namespace {

// One call: gft_series_args.hpp judges it (everything that touches no device state, around the pointer check it is handed) and
// collapses the batch; what is left here needs the device -- the factor table, the workspace, the stream joins and the dispatch.
static int series_call(const gft::SeriesCall& c, void* stream) {
    const std::string f(c.fn);
    gft::SeriesArgs a;
    if (!gft::series_args(c, a, [&](const double* p, const char* what) { check_device_ptr(p, (f + ": " + what).c_str()); })) return 0;
    const int op = c.op, w = c.w;
    const double *x = c.x.p, *y = c.y.p;
    double* res = const_cast<double*>(c.r.p);
    const gft::SeriesItem& it = a.it;
    const gft::SeriesBatch& g = a.g;
    const gft::SeriesPlanes& pl = a.pl;
    const hipStream_t cs = (hipStream_t)stream;
    const gft::SeriesOpRow& row = gft::series_op_row(op);
    switch (row.family) {
    case gft::SERIES_CHAIN: {  // one launch for the whole chain; the derivative's factors of order 1 over the axis
        const size_t tlen = (c.rank == 2 && c.var == 0 ? it.nx[1] : it.nx[2]) - 1;
        Rc<Buf> tab = w == 2 ? Ops<EIv>::cached_table(TAB_DERIV, 1, tlen) : Ops<EF64>::cached_table(TAB_DERIV, 1, tlen);
        join_caller_in(cs);
        if (op == gft::SERIES_OBSERVE_NEGBINOMIAL) {  // the same table; p travels beside the batch
            R.series_last = gft::series_observe_negbinomial(R.stream, x, y, c.p.p, a.ps, a.pp, c.cs.p, res, gft::series2_dims(it), c.var, c.rank == 2,
                                                            (unsigned)(c.cs.len[2] - 1), (unsigned)c.degree_p1, g, pl, tab->p, tlen, R.series_force);
            join_caller_out(cs);
            return 0;
        }
        R.series_last = gft::series_observe_chain(R.stream, x, y, c.cs.p, res, gft::series2_dims(it), c.var, c.rank == 2, (unsigned)c.nsteps,
                                                  (unsigned)c.degree_p1, g, pl, tab->p, tlen, R.series_force);
        join_caller_out(cs);
        return 0;
    }
    case gft::SERIES_LINEAR: {  // one launch; c and m travel as the chain's x and cs
        join_caller_in(cs);
        R.series_last = gft::series_linear(R.stream, op, x, y, c.cs.p, res, gft::series2_dims(it), c.var, c.wvar, g, pl, R.series_force);
        join_caller_out(cs);
        return 0;
    }
    case gft::SERIES_OBSERVE: {
        if (op == gft::SERIES_LAH_ROW) {  // no table: the row is a recurrence on the item's own p
            join_caller_in(cs);
            R.series_last = gft::series_lah_row(R.stream, x, res, (unsigned)(c.r.len[2] - 1), g, pl, R.series_force);
            join_caller_out(cs);
            return 0;
        }
        // the factors depend on (op, k, len) only: computed once with the reference's rounding (k_factor_table's functor) and kept.
        // A table is written on the library's stream, where the kernel below runs: its first use is ordered behind it.
        Rc<Buf> tab;
        size_t tlen = 0;
        if (op == gft::SERIES_DERIVATIVE || op == gft::SERIES_COEFF) {
            tlen = c.rank == 2 && c.var == 0 ? it.n[1] : it.n[2];
            const int top = op == gft::SERIES_DERIVATIVE ? TAB_DERIV : TAB_COEFF;
            tab = w == 2 ? Ops<EIv>::cached_table(top, c.k, tlen) : Ops<EF64>::cached_table(top, c.k, tlen);
        }
        join_caller_in(cs);
        gft::series_observe(R.stream, op, x, res, gft::series2_dims(it), c.var, (unsigned)c.k, g, pl, tab ? tab->p : nullptr, tlen, c.rank == 2);
        join_caller_out(cs);
        R.series_last = gft::SERIES_NONE;
        return 0;
    }
    case gft::SERIES_POWER: {  // one driver for every rank
        Rc<Buf> ws = alloc_doubles(gft::series_pow_workspace(g.items, it.n, w));  // (returned to the pool on exit: later launches follow)
        join_caller_in(cs);
        R.series_last = gft::series_pow(R.stream, c.rank, x, c.e, res, it, g, ws->p, R.series_force, pl);
        join_caller_out(cs);
        return 0;
    }
    case gft::SERIES_ARITH: break;  // by the rank, below
    }
    // ranks 2 and 3 have one form, planned before the streams are joined (the planner may refuse)
    if (c.rank == 3) {  // on the permuted item of the stored result shape S (compose: of the chain's final shape)
        if (op == gft::SERIES_COMPOSE) {
            const gft::Series3Compose k = gft::series3_compose_dims(it, c.var);
            const gft::Series3Plan plan = gft::series3_compose_plan(k, w);
            join_caller_in(cs);
            gft::series3_compose_launch(R.stream, plan, x, y, res, k, g, pl);
        } else {
            const gft::Series3Dims k = gft::series3_dims(op, it);
            const gft::Series3Plan plan = gft::series3_plan(op, k, w);
            join_caller_in(cs);
            gft::series3_launch(R.stream, op, plan, x, y, res, k, g, pl);
        }
        join_caller_out(cs);
        R.series_last = gft::SERIES_FORM_B;
        return 0;
    }
    if (c.rank == 2) {
        const gft::Series2Dims d = gft::series2_dims(it);
        const gft::Series2Plan plan = gft::series2_plan(op, d, w);
        join_caller_in(cs);
        gft::series2_launch(R.stream, op, plan, x, y, res, d, g, c.var, pl);
        join_caller_out(cs);
        R.series_last = gft::SERIES_FORM_B;
        return 0;
    }
    const unsigned nx = it.nx[2], ny = it.ny[2], n = it.n[2];
    const int form = gft::series_plan(op, g.items, row.xlong ? nx : n, R.series_force, w, c.elem);  // (the planner sizes the long rows)
    const size_t wsn = gft::series_workspace(op, form, g.items, nx, n, w);
    Rc<Buf> ws;
    if (wsn) ws = alloc_doubles(wsn);  // (returned to the pool on exit: later launches follow these on the one stream)
    join_caller_in(cs);
    gft::series_launch(R.stream, op, form, x, nx, y, ny, res, n, g, wsn ? ws->p : nullptr, pl);
    join_caller_out(cs);
    R.series_last = form;
    return 0;
}

// an operand as the entry points receive it, from the unit-stride axis outwards: its length, then stride and length of the row axis
// (rank 2 up) and of the slab axis (rank 3)
static gft::SeriesView view(const double* p, const int64_t* bs, size_t len2, int64_t rst = 0, size_t len1 = 1, int64_t sst = 0, size_t len0 = 1) {
    gft::SeriesView v;
    v.p = p, v.bs = bs;
    v.st[0] = sst, v.st[1] = rst;
    v.len[0] = len0, v.len[1] = len1, v.len[2] = len2;
    return v;
}

}  // namespace

// An entry point: the descriptor `c` with the call's common fields, FILL names the rest (the operands, e, var, k).  ELEM: what the W
// planes hold (gft::SeriesElem); the entry points without one take it from the width.
#define GFT_SERIES_ENTRY_ELEM(OP, FN, W, ELEM, RANK, FILL)                         \
    return guard_int([&] {                                                         \
        gft::SeriesCall c;                                                         \
        c.op = gft::OP, c.fn = FN, c.w = W, c.elem = gft::ELEM, c.rank = RANK, c.batch = batch, c.nbatch = nbatch; \
        FILL;                                                                      \
        return series_call(c, stream);                                             \
    })
#define GFT_SERIES_ENTRY(OP, FN, W, RANK, FILL) GFT_SERIES_ENTRY_ELEM(OP, FN, W, SERIES_ELEM_BY_WIDTH, RANK, FILL)
// the argument lists the arithmetic ops share: two operands (at rank 2 with or without compose's var), an operand and its seeds
#define GFT_SERIES_BINARY_ELEM(SYM, OP, FN, W, ELEM)                                                                                          \
    int SYM(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny, double* res, const int64_t* rbs,  \
            size_t n, const size_t* batch, size_t nbatch, void* stream) {                                                                     \
        GFT_SERIES_ENTRY_ELEM(OP, FN, W, ELEM, 1, (c.x = view(x, xbs, nx), c.y = view(y, ybs, ny), c.r = view(res, rbs, n)));                 \
    }
#define GFT_SERIES_BINARY(SYM, OP, FN, W) GFT_SERIES_BINARY_ELEM(SYM, OP, FN, W, SERIES_ELEM_BY_WIDTH)
#define GFT_SERIES_SEEDED_ELEM(SYM, OP, FN, W, ELEM)                                                                                          \
    int SYM(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs, double* res, const int64_t* rbs, size_t n, \
            const size_t* batch, size_t nbatch, void* stream) {                                                                               \
        GFT_SERIES_ENTRY_ELEM(OP, FN, W, ELEM, 1, (c.x = view(x, xbs, nx), c.y = view(seed, sbs, 1), c.r = view(res, rbs, n)));               \
    }
#define GFT_SERIES2_BINARY(SYM, OP, FN, W)                                                                                                    \
    int SYM(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs, int64_t yrs,       \
            size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,   \
            void* stream) {                                                                                                                   \
        GFT_SERIES_ENTRY(OP, FN, W, 2,                                                                                                        \
                         (c.x = view(x, xbs, nx1, xrs, nx0), c.y = view(y, ybs, ny1, yrs, ny0), c.r = view(res, rbs, n1, rrs, n0)));          \
    }
#define GFT_SERIES2_BINARY_VAR(SYM, OP, FN, W)                                                                                                \
    int SYM(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs, int64_t yrs,       \
            size_t ny0, size_t ny1, int var, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch,         \
            size_t nbatch, void* stream) {                                                                                                    \
        GFT_SERIES_ENTRY(OP, FN, W, 2,                                                                                                        \
                         (c.x = view(x, xbs, nx1, xrs, nx0), c.y = view(y, ybs, ny1, yrs, ny0), c.var = var,                                  \
                          c.r = view(res, rbs, n1, rrs, n0)));                                                                                \
    }
#define GFT_SERIES2_SEEDED(SYM, OP, FN, W)                                                                                                    \
    int SYM(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* seed, const int64_t* sbs, double* res,    \
            const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {                        \
        GFT_SERIES_ENTRY(OP, FN, W, 2, (c.x = view(x, xbs, nx1, xrs, nx0), c.y = view(seed, sbs, 1), c.r = view(res, rbs, n1, rrs, n0)));     \
    }
// rank 3: a slab stride and a row stride per operand, three lengths
#define GFT_SERIES3_BINARY(SYM, OP, FN, W)                                                                                                    \
    int SYM(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* y,               \
            const int64_t* ybs, int64_t yss, int64_t yrs, size_t ny0, size_t ny1, size_t ny2, double* res, const int64_t* rbs, int64_t rss,   \
            int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch, size_t nbatch, void* stream) {                                 \
        GFT_SERIES_ENTRY(OP, FN, W, 3,                                                                                                        \
                         (c.x = view(x, xbs, nx2, xrs, nx1, xss, nx0), c.y = view(y, ybs, ny2, yrs, ny1, yss, ny0),                           \
                          c.r = view(res, rbs, n2, rrs, n1, rss, n0)));                                                                       \
    }
#define GFT_SERIES3_SEEDED(SYM, OP, FN, W)                                                                                                    \
    int SYM(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* seed,            \
            const int64_t* sbs, double* res, const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2,                   \
            const size_t* batch, size_t nbatch, void* stream) {                                                                               \
        GFT_SERIES_ENTRY(OP, FN, W, 3,                                                                                                        \
                         (c.x = view(x, xbs, nx2, xrs, nx1, xss, nx0), c.y = view(seed, sbs, 1),                                              \
                          c.r = view(res, rbs, n2, rrs, n1, rss, n0)));                                                                       \
    }
#define GFT_SERIES3_COMPOSE_POW(PFX, WHAT, W)                                                                                                 \
    int PFX##series3_compose(const double* f, const int64_t* fbs, int64_t fss, int64_t frs, size_t nf0, size_t nf1, size_t nf2, const double* g, \
                            const int64_t* gbs, int64_t gss, int64_t grs, size_t ng0, size_t ng1, size_t ng2, int var, double* res,           \
                            const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch, size_t nbatch, \
                            void* stream) {                                                                                                   \
        GFT_SERIES_ENTRY(SERIES_COMPOSE, WHAT "series3_compose", W, 3,                                                                        \
                         (c.x = view(f, fbs, nf2, frs, nf1, fss, nf0), c.y = view(g, gbs, ng2, grs, ng1, gss, ng0),                           \
                          c.var = var, c.r = view(res, rbs, n2, rrs, n1, rss, n0)));                                                          \
    }                                                                                                                                         \
    int PFX##series3_pow(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, uint32_t e,       \
                        double* res, const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch,      \
                        size_t nbatch, void* stream) {                                                                                        \
        GFT_SERIES_ENTRY(SERIES_POW, WHAT "series3_pow", W, 3,                                                                                \
                         (c.x = view(x, xbs, nx2, xrs, nx1, xss, nx0), c.e = e, c.r = view(res, rbs, n2, rrs, n1, rss, n0)));                 \
    }
#define GFT_SERIES3_ARITH(PFX, WHAT, W)                                        \
    GFT_SERIES3_BINARY(PFX##series3_mul, SERIES_MUL, WHAT "series3_mul", W)    \
    GFT_SERIES3_BINARY(PFX##series3_div, SERIES_DIV, WHAT "series3_div", W)    \
    GFT_SERIES3_SEEDED(PFX##series3_exp, SERIES_EXP, WHAT "series3_exp", W)    \
    GFT_SERIES3_SEEDED(PFX##series3_log, SERIES_LOG, WHAT "series3_log", W)    \
    GFT_SERIES3_COMPOSE_POW(PFX, WHAT, W)
// The arithmetic ops at both ranks.  Interval<F64> (gfti_, W == 2): the same calls on (lo, hi) planes; every batch-stride array has
// nbatch + 1 entries, the plane stride first.  Rank 2: the last two axes are an item's coefficient array, with a row stride each.
// (rank 1 is its own macro: the BigFloat family has no other rank)
#define GFT_SERIES1_ARITH(PFX, WHAT, W, ELEM)                                                                                                 \
    GFT_SERIES_BINARY_ELEM(PFX##series_mul, SERIES_MUL, WHAT "series_mul", W, ELEM)                                                           \
    GFT_SERIES_BINARY_ELEM(PFX##series_div, SERIES_DIV, WHAT "series_div", W, ELEM)                                                           \
    GFT_SERIES_SEEDED_ELEM(PFX##series_exp, SERIES_EXP, WHAT "series_exp", W, ELEM)                                                           \
    GFT_SERIES_SEEDED_ELEM(PFX##series_log, SERIES_LOG, WHAT "series_log", W, ELEM)                                                           \
    GFT_SERIES_BINARY_ELEM(PFX##series_compose, SERIES_COMPOSE, WHAT "series_compose", W, ELEM)                                               \
    int PFX##series_pow(const double* x, const int64_t* xbs, size_t nx, uint32_t e, double* res, const int64_t* rbs, size_t n,                \
                        const size_t* batch, size_t nbatch, void* stream) {                                                                   \
        GFT_SERIES_ENTRY_ELEM(SERIES_POW, WHAT "series_pow", W, ELEM, 1, (c.x = view(x, xbs, nx), c.e = e, c.r = view(res, rbs, n)));         \
    }
#define GFT_SERIES_ARITH(PFX, WHAT, W)                                                                                                        \
    GFT_SERIES1_ARITH(PFX, WHAT, W, SERIES_ELEM_BY_WIDTH)                                                                                     \
    GFT_SERIES2_BINARY(PFX##series2_mul, SERIES_MUL, WHAT "series2_mul", W)                                                                   \
    GFT_SERIES2_BINARY(PFX##series2_div, SERIES_DIV, WHAT "series2_div", W)                                                                   \
    GFT_SERIES2_SEEDED(PFX##series2_exp, SERIES_EXP, WHAT "series2_exp", W)                                                                   \
    GFT_SERIES2_SEEDED(PFX##series2_log, SERIES_LOG, WHAT "series2_log", W)                                                                   \
    GFT_SERIES2_BINARY_VAR(PFX##series2_compose, SERIES_COMPOSE, WHAT "series2_compose", W)                                                   \
    int PFX##series2_pow(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, uint32_t e, double* res,                   \
                         const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {           \
        GFT_SERIES_ENTRY(SERIES_POW, WHAT "series2_pow", W, 2, (c.x = view(x, xbs, nx1, xrs, nx0), c.e = e, c.r = view(res, rbs, n1, rrs, n0))); \
    }
// the observation ops: one operand, the order k (at rank 2 behind the variable), the result k shorter on that axis
#define GFT_SERIES_OBSERVE_K(PFX, NAME, OP, WHAT, W)                                                                                          \
    int PFX##series_##NAME(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs, size_t n,               \
                           const size_t* batch, size_t nbatch, void* stream) {                                                                \
        GFT_SERIES_ENTRY(OP, WHAT "series_" #NAME, W, 1, (c.x = view(x, xbs, nx), c.var = 1, c.k = k, c.r = view(res, rbs, n)));              \
    }                                                                                                                                         \
    int PFX##series2_##NAME(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k, double* res,         \
                            const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {        \
        GFT_SERIES_ENTRY(OP, WHAT "series2_" #NAME, W, 2,                                                                                     \
                         (c.x = view(x, xbs, nx1, xrs, nx0), c.var = var, c.k = k, c.r = view(res, rbs, n1, rrs, n0)));                       \
    }
#define GFT_SERIES_OBSERVE(PFX, WHAT, W)                                                                                                      \
    GFT_SERIES_OBSERVE_K(PFX, derivative, SERIES_DERIVATIVE, WHAT, W)                                                                         \
    GFT_SERIES_OBSERVE_K(PFX, taylor_expansion_of_coeff, SERIES_COEFF, WHAT, W)                                                               \
    GFT_SERIES_OBSERVE_K(PFX, shift_down, SERIES_SHIFT_DOWN, WHAT, W)                                                                         \
    int PFX##series_evaluate_all_one(const double* x, const int64_t* xbs, size_t nx, double* res, const int64_t* rbs, const size_t* batch,    \
                                     size_t nbatch, void* stream) {                                                                           \
        GFT_SERIES_ENTRY(SERIES_EVAL_ONE, WHAT "series_evaluate_all_one", W, 1, (c.x = view(x, xbs, nx), c.var = 1, c.r = view(res, rbs, 1))); \
    }                                                                                                                                         \
    int PFX##series2_evaluate_all_one(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, double* res,                  \
                                      const int64_t* rbs, const size_t* batch, size_t nbatch, void* stream) {                                 \
        GFT_SERIES_ENTRY(SERIES_EVAL_ONE, WHAT "series2_evaluate_all_one", W, 2, (c.x = view(x, xbs, nx1, xrs, nx0), c.r = view(res, rbs, 1))); \
    }
// the fused observation chain: the operand a (at rank 2 with the axis), the scalars x (NULL: the continuous form) and the constants
// cs of every item, then the result with degree_p1 coefficients on the axis
#define GFT_SERIES_OBSERVE_CHAIN(PFX, WHAT, W)                                                                                                \
    int PFX##series_observe_chain(const double* a, const int64_t* abs, size_t na, const double* x, const int64_t* xbs, const double* cs,      \
                                  const int64_t* cbs, size_t nsteps, size_t degree_p1, double* res, const int64_t* rbs, size_t n,             \
                                  const size_t* batch, size_t nbatch, void* stream) {                                                         \
        GFT_SERIES_ENTRY(SERIES_OBSERVE_CHAIN, WHAT "series_observe_chain", W, 1,                                                             \
                         (c.x = view(a, abs, na), c.var = 1, c.y = view(x, xbs, 1), c.cs = view(cs, cbs, nsteps), c.nsteps = nsteps,          \
                          c.degree_p1 = degree_p1, c.r = view(res, rbs, n)));                                                                 \
    }                                                                                                                                         \
    int PFX##series2_observe_chain(const double* a, const int64_t* abs, int64_t ars, size_t na0, size_t na1, int var, const double* x,        \
                                   const int64_t* xbs, const double* cs, const int64_t* cbs, size_t nsteps, size_t degree_p1, double* res,    \
                                   const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) { \
        GFT_SERIES_ENTRY(SERIES_OBSERVE_CHAIN, WHAT "series2_observe_chain", W, 2,                                                            \
                         (c.x = view(a, abs, na1, ars, na0), c.var = var, c.y = view(x, xbs, 1), c.cs = view(cs, cbs, nsteps),                \
                          c.nsteps = nsteps, c.degree_p1 = degree_p1, c.r = view(res, rbs, n1, rrs, n0)));                                    \
    }
// the negative-binomial observation: the operand a (at rank 2 with the axis), the scalars x and p and the row ls (order + 1 entries)
// of every item, then the result with degree_p1 coefficients on the axis; and the row itself from p
#define GFT_SERIES_OBSERVE_NEGBINOMIAL(PFX, WHAT, W)                                                                                          \
    int PFX##series_observe_negbinomial(const double* a, const int64_t* abs, size_t na, const double* x, const int64_t* xbs, const double* p,  \
                                        const int64_t* pbs, const double* ls, const int64_t* lbs, size_t nls, size_t degree_p1, double* res,  \
                                        const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {                     \
        GFT_SERIES_ENTRY(SERIES_OBSERVE_NEGBINOMIAL, WHAT "series_observe_negbinomial", W, 1,                                                 \
                         (c.x = view(a, abs, na), c.var = 1, c.y = view(x, xbs, 1), c.p = view(p, pbs, 1), c.cs = view(ls, lbs, nls),         \
                          c.nsteps = nls, c.degree_p1 = degree_p1, c.r = view(res, rbs, n)));                                                 \
    }                                                                                                                                         \
    int PFX##series2_observe_negbinomial(const double* a, const int64_t* abs, int64_t ars, size_t na0, size_t na1, int var, const double* x,  \
                                         const int64_t* xbs, const double* p, const int64_t* pbs, const double* ls, const int64_t* lbs,       \
                                         size_t nls, size_t degree_p1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1,    \
                                         const size_t* batch, size_t nbatch, void* stream) {                                                  \
        GFT_SERIES_ENTRY(SERIES_OBSERVE_NEGBINOMIAL, WHAT "series2_observe_negbinomial", W, 2,                                                \
                         (c.x = view(a, abs, na1, ars, na0), c.var = var, c.y = view(x, xbs, 1), c.p = view(p, pbs, 1),                       \
                          c.cs = view(ls, lbs, nls), c.nsteps = nls, c.degree_p1 = degree_p1, c.r = view(res, rbs, n1, rrs, n0)));            \
    }                                                                                                                                         \
    int PFX##series_lah_row(const double* p, const int64_t* pbs, size_t order, double* res, const int64_t* rbs, const size_t* batch,          \
                            size_t nbatch, void* stream) {                                                                                    \
        GFT_SERIES_ENTRY(SERIES_LAH_ROW, WHAT "series_lah_row", W, 1, (c.x = view(p, pbs, 1), c.var = 1, c.r = view(res, rbs, order + 1)));   \
    }
// the affine substitutions: the operand (at rank 2 with var, compose_linear also with wvar), the scalars c and m of every item, then
// the result
#define GFT_SERIES_LINEAR(PFX, WHAT, W)                                                                                                       \
    int PFX##series_mul_linear(const double* a, const int64_t* abs, size_t na, const double* cv, const int64_t* cbs, const double* mv,         \
                               const int64_t* mbs, double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch,             \
                               void* stream) {                                                                                                \
        GFT_SERIES_ENTRY(SERIES_MUL_LINEAR, WHAT "series_mul_linear", W, 1,                                                                   \
                         (c.x = view(a, abs, na), c.var = 1, c.wvar = 1, c.y = view(cv, cbs, 1), c.cs = view(mv, mbs, 1), c.r = view(res, rbs, n))); \
    }                                                                                                                                         \
    int PFX##series2_mul_linear(const double* a, const int64_t* abs, int64_t ars, size_t na0, size_t na1, int var, const double* cv,          \
                                const int64_t* cbs, const double* mv, const int64_t* mbs, double* res, const int64_t* rbs, int64_t rrs,        \
                                size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {                                     \
        GFT_SERIES_ENTRY(SERIES_MUL_LINEAR, WHAT "series2_mul_linear", W, 2,                                                                  \
                         (c.x = view(a, abs, na1, ars, na0), c.var = var, c.wvar = var, c.y = view(cv, cbs, 1), c.cs = view(mv, mbs, 1),        \
                          c.r = view(res, rbs, n1, rrs, n0)));                                                                                \
    }                                                                                                                                         \
    int PFX##series_compose_linear(const double* f, const int64_t* fbs, size_t nf, const double* cv, const int64_t* cbs, const double* mv,     \
                                   const int64_t* mbs, double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch,         \
                                   void* stream) {                                                                                            \
        GFT_SERIES_ENTRY(SERIES_COMPOSE_LINEAR, WHAT "series_compose_linear", W, 1,                                                           \
                         (c.x = view(f, fbs, nf), c.var = 1, c.wvar = 1, c.y = view(cv, cbs, 1), c.cs = view(mv, mbs, 1), c.r = view(res, rbs, n))); \
    }                                                                                                                                         \
    int PFX##series2_compose_linear(const double* f, const int64_t* fbs, int64_t frs, size_t nf0, size_t nf1, int var, int wvar,              \
                                    const double* cv, const int64_t* cbs, const double* mv, const int64_t* mbs, double* res,                    \
                                    const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) { \
        GFT_SERIES_ENTRY(SERIES_COMPOSE_LINEAR, WHAT "series2_compose_linear", W, 2,                                                          \
                         (c.x = view(f, fbs, nf1, frs, nf0), c.var = var, c.wvar = wvar, c.y = view(cv, cbs, 1), c.cs = view(mv, mbs, 1),       \
                          c.r = view(res, rbs, n1, rrs, n0)));                                                                                \
    }

extern "C" {
GFT_SERIES_LINEAR(gft_, "", 1)
GFT_SERIES_LINEAR(gfti_, "interval ", 2)
GFT_SERIES_OBSERVE_CHAIN(gft_, "", 1)
GFT_SERIES_OBSERVE_CHAIN(gfti_, "interval ", 2)
GFT_SERIES_OBSERVE_NEGBINOMIAL(gft_, "", 1)
GFT_SERIES_OBSERVE_NEGBINOMIAL(gfti_, "interval ", 2)
GFT_SERIES_ARITH(gft_, "", 1)
GFT_SERIES_ARITH(gfti_, "interval ", 2)
// BigFloat (gftb_, W == 2 planes: factor, exponent): rank 1's six arithmetic operations and nothing else
GFT_SERIES1_ARITH(gftb_, "bigfloat ", 2, SERIES_ELEM_BIGFLOAT)
GFT_SERIES_OBSERVE(gft_, "", 1)
GFT_SERIES_OBSERVE(gfti_, "interval ", 2)
// the transposed operations (f64 only): g / gh is the long side, the result the short one
GFT_SERIES_BINARY(gft_series_corr, SERIES_CORR, "series_corr", 1)
GFT_SERIES_BINARY(gft_series_compose_adj, SERIES_COMPOSE_ADJ, "series_compose_adj", 1)
GFT_SERIES2_BINARY(gft_series2_corr, SERIES_CORR, "series2_corr", 1)
GFT_SERIES2_BINARY_VAR(gft_series2_compose_adj, SERIES_COMPOSE_ADJ, "series2_compose_adj", 1)
GFT_SERIES3_ARITH(gft_, "", 1)
GFT_SERIES3_ARITH(gfti_, "interval ", 2)
int gft_series_last_form(void) { return R.series_last; }
}
#undef GFT_SERIES_ENTRY_ELEM
#undef GFT_SERIES_ENTRY
#undef GFT_SERIES_BINARY_ELEM
#undef GFT_SERIES_BINARY
#undef GFT_SERIES_SEEDED_ELEM
#undef GFT_SERIES1_ARITH
#undef GFT_SERIES2_BINARY
#undef GFT_SERIES2_BINARY_VAR
#undef GFT_SERIES2_SEEDED
#undef GFT_SERIES3_BINARY
#undef GFT_SERIES3_SEEDED
#undef GFT_SERIES3_COMPOSE_POW
#undef GFT_SERIES3_ARITH
#undef GFT_SERIES_ARITH
#undef GFT_SERIES_OBSERVE_CHAIN
#undef GFT_SERIES_OBSERVE_NEGBINOMIAL
#undef GFT_SERIES_LINEAR
#undef GFT_SERIES_OBSERVE_K
#undef GFT_SERIES_OBSERVE
