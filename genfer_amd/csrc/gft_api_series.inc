// ------------------------------------------------------------------------------------------
// batched univariate series on caller-owned device tensors: gft_series_mul / div / exp / log / compose / pow / corr / compose_adj,
// and the first six's Interval<F64> twins gfti_series_* (w == 2: every stride array starts with the lo -> hi plane stride)
// and the bivariate gft_series2_mul / div / exp / log / compose / pow with their Interval<F64> twins gfti_series2_* (the same
// validation with one row stride per operand: series2_call), and the f64-only transposed gft_series2_corr / compose_adj
// and the observation ops gft_series_* / gft_series2_* derivative / taylor_expansion_of_coeff / shift_down / evaluate_all_one with
// their gfti_ twins (one operand, the result shorter by the order k on one axis; the kernels: gft_series_observe.hip)
// (the planner and the kernels: gft_series.hpp, gft_series.hip; included by gft_api.hip after the device interop, whose
// pointer check and stream joins it shares)
// ------------------------------------------------------------------------------------------
namespace {

struct SeriesArg {  // one operand of a call: rows of `len` elements (unit stride), batch strides in elements
    const char* what;
    const double* p;
    size_t len;
    size_t rows, rst;  // rank 2 (gft_series2_*): an item is `rows` such rows, `rst` elements apart; else 1 and 0
    size_t st[32];
    size_t plane;  // w == 2: elements from the lo plane to the hi plane (0 on an operand: a point interval), else 0
    size_t span;   // elements from p to one past its last element (of the hi plane)
};

// `bs`: nbatch strides, for w == 2 preceded by the plane stride.  rank 2: `rows` rows per item, `rst` elements apart.
static SeriesArg series_arg(const char* fn, const char* what, const double* p, const int64_t* bs, size_t len, const size_t* batch, size_t nbatch,
                            int w, size_t rows = 1, int64_t rst = 0) {
    SeriesArg a;
    a.what = what;
    a.p = p;
    a.len = len;
    if (rst < 0) throw Error(std::string(fn) + ": negative strides are not supported (" + what + ", the row axis)");
    a.rows = rows;
    a.rst = rows > 1 ? (size_t)rst : 0;
    size_t cs = len * rows;  // NULL: contiguous items of the operand's own shape (the planes back to back)
    a.span = len + (rows - 1) * a.rst;
    if (w == 2 && bs) {
        if (bs[0] < 0) throw Error(std::string(fn) + ": negative strides are not supported (" + what + ", the plane axis)");
        ++bs;
    }
    for (size_t i = nbatch; i-- > 0;) {
        if (bs && bs[i] < 0)
            throw Error(std::string(fn) + ": negative strides are not supported (" + what + ", batch axis " + std::to_string(i) + ")");
        a.st[i] = bs ? (size_t)bs[i] : cs;
        cs *= batch[i];
        a.span += (batch[i] - 1) * a.st[i];
    }
    a.plane = w == 2 ? (bs ? (size_t)bs[-1] : cs) : 0;
    a.span += a.plane;
    return a;
}

static bool series_same_view(const SeriesArg& a, const SeriesArg& b, const size_t* batch, size_t nbatch) {
    if (a.p != b.p || a.len != b.len || a.plane != b.plane || a.rows != b.rows || a.rst != b.rst) return false;
    for (size_t i = 0; i < nbatch; ++i)
        if (batch[i] > 1 && a.st[i] != b.st[i]) return false;
    return true;
}

// `y`: the second operand (mul, div; compose: x is f, y is g) or the seeds (exp, log; may be null); pow has neither, and `e`.
// corr (x is g, y is y, n is m) and compose_adj (x is gh, y is g, n is nf) are the transposed operations: their result is the SHORT
// side, so nx bounds n and ny, and the rows the planner sizes are the nx long ones.
// `d2` (gft_series2_*, gfti_series2_*): the call is at rank 2 -- nx, ny, n are the lengths along the series axis (d2->nx1, ny1, n1), an
// item has d2->nx0 / ny0 / n0 rows d2->xr / yr / rr elements apart, and the limit bounds n0 * n1.  `var`: compose's variable there.
// The observation ops (SERIES_DERIVATIVE ...): x is the one operand and the LONG side, `k` the order, `var` the axis at rank 2 (at
// rank 1 the callers pass 1, the series axis), and the result's shape must be x's with k taken off that axis (evaluate_all_one: one
// element per item).  The limits bound x's stored shape.
static int series_call(int op, const char* fn, const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny,
                       double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream, uint32_t e = 0, int w = 1,
                       const gft::Series2Dims* d2 = nullptr, const int64_t* rowst = nullptr, int var = 0, size_t k = 0) {
    const bool observe = op >= gft::SERIES_DERIVATIVE;
    const bool corr = op == gft::SERIES_CORR, adj = op == gft::SERIES_COMPOSE_ADJ, transposed = corr || adj;
    const bool binary = op == gft::SERIES_MUL || op == gft::SERIES_DIV || op == gft::SERIES_COMPOSE || transposed;
    const std::string f(fn);
    size_t x0 = 1, y0 = 1, r0 = 1;  // rows per item
    if (observe) {
        x0 = d2 ? d2->nx0 : 1, r0 = d2 ? d2->n0 : 1;
        if (x0 == 0 || nx == 0) throw Error(f + ": x has no coefficients");
        if (d2) {
            const size_t most = gft::series2_max_elems(w);
            if (x0 > most || nx > most || x0 * nx > most)
                throw Error(f + ": x has " + std::to_string(x0) + " * " + std::to_string(nx) + " coefficients, which exceeds the limit of " +
                            std::to_string(most) + " coefficients per item of this version");
            if (var != 0 && var != 1) throw Error(f + ": var = " + std::to_string(var) + " (the variable the operation acts on is 0 or 1)");
        } else if (nx > gft::series_max_n(w))
            throw Error(f + ": nx = " + std::to_string(nx) + " exceeds the limit of " + std::to_string(gft::series_max_n(w)) + " coefficients per series of this version");
        if (op != gft::SERIES_EVAL_ONE) {
            const bool rows = d2 && var == 0;
            const size_t len = rows ? x0 : nx;
            if (k >= len)
                throw Error(f + ": k = " + std::to_string(k) + ", but x has " + std::to_string(len) + " stored coefficients" +
                            (d2 ? " on axis " + std::to_string(var) : std::string()) + " (the order must satisfy 0 <= k < " + std::to_string(len) + ")");
            const size_t w0 = rows ? x0 - k : x0, w1 = rows ? nx : nx - k;
            if (r0 != w0 || n != w1)
                throw Error(f + ": the result has " + (d2 ? std::to_string(r0) + " x " : std::string()) + std::to_string(n) + " coefficients; with k = " +
                            std::to_string(k) + " it has " + (d2 ? std::to_string(w0) + " x " : std::string()) + std::to_string(w1) + " (x's, less k on the axis)");
        }
    } else if (d2 && transposed) {  // x (g, gh) is the long side on both axes: it carries the limit and bounds y and the result
        x0 = d2->nx0, y0 = d2->ny0, r0 = d2->n0;
        const std::string xn = corr ? "g" : "gh", yn = corr ? "y" : "g";
        if (r0 == 0 || n == 0) throw Error(f + ": the result has no coefficients (an axis of its shape is 0)");
        const size_t most = gft::series2_max_elems(w);
        if (x0 > most || nx > most || x0 * nx > most)
            throw Error(f + ": " + xn + " has " + std::to_string(x0) + " * " + std::to_string(nx) + " coefficients, which exceeds the limit of " +
                        std::to_string(most) + " coefficients per item of this version");
        if (x0 == 0 || nx == 0 || y0 == 0 || ny == 0) throw Error(f + ": an operand has no coefficients");
        if (r0 > x0 || n > nx)
            throw Error(f + ": the result has " + std::to_string(r0) + " x " + std::to_string(n) + " coefficients, " + xn + " " + std::to_string(x0) + " x " +
                        std::to_string(nx) + " (the result of a transposed operation is its short side)");
        if (y0 > x0 || ny > nx)
            throw Error(f + ": " + yn + " has " + std::to_string(y0) + " x " + std::to_string(ny) + " coefficients, " + xn + " " + std::to_string(x0) + " x " +
                        std::to_string(nx) + " (an operand is longer than the truncation order)");
    } else if (d2) {
        x0 = d2->nx0, y0 = binary ? d2->ny0 : 1, r0 = d2->n0;
        if (r0 == 0 || n == 0) throw Error(f + ": n0 * n1 == 0 (the result has no coefficients)");
        const size_t most = gft::series2_max_elems(w);
        if (r0 > most || n > most || r0 * n > most)
            throw Error(f + ": n0 * n1 = " + std::to_string(r0) + " * " + std::to_string(n) + " exceeds the limit of " + std::to_string(most) +
                        " coefficients per item of this version");
        if (x0 == 0 || nx == 0 || (binary && (y0 == 0 || ny == 0))) throw Error(f + ": an operand has no coefficients");
        if (x0 > r0 || nx > n)
            throw Error(f + ": x has " + std::to_string(x0) + " x " + std::to_string(nx) + " coefficients, the result " + std::to_string(r0) + " x " + std::to_string(n) +
                        " (an operand is longer than the truncation order)");
        if (binary && (y0 > r0 || ny > n))
            throw Error(f + ": y has " + std::to_string(y0) + " x " + std::to_string(ny) + " coefficients, the result " + std::to_string(r0) + " x " + std::to_string(n) +
                        " (an operand is longer than the truncation order)");
    } else if (transposed) {
        const char* nl = corr ? "ng" : "n";   // the long side (x)
        const char* ns = corr ? "ny" : "ng";  // the second operand
        const char* nr = corr ? "m" : "nf";   // the result
        if (n == 0) throw Error(f + ": " + nr + " == 0 (the result has no coefficients)");
        if (nx > gft::series_max_n(w))
            throw Error(f + ": " + nl + " = " + std::to_string(nx) + " exceeds the limit of " + std::to_string(gft::series_max_n(w)) + " coefficients per series of this version");
        if (nx == 0 || ny == 0) throw Error(f + ": an operand has no coefficients");
        if (n > nx) throw Error(f + ": " + nr + " = " + std::to_string(n) + " > " + nl + " = " + std::to_string(nx) + " (the result of a transposed operation is its short side)");
        if (ny > nx) throw Error(f + ": " + ns + " = " + std::to_string(ny) + " > " + nl + " = " + std::to_string(nx) + " (an operand is longer than the truncation order)");
    } else {
        if (n == 0) throw Error(f + ": n == 0 (the result has no coefficients)");
        if (n > gft::series_max_n(w))
            throw Error(f + ": n = " + std::to_string(n) + " exceeds the limit of " + std::to_string(gft::series_max_n(w)) + " coefficients per series of this version");
        if (nx == 0 || (binary && ny == 0)) throw Error(f + ": an operand has no coefficients");
        if (nx > n) throw Error(f + ": nx = " + std::to_string(nx) + " > n = " + std::to_string(n) + " (an operand is longer than the truncation order)");
        if (binary && ny > n) throw Error(f + ": ny = " + std::to_string(ny) + " > n = " + std::to_string(n) + " (an operand is longer than the truncation order)");
    }
    if (nbatch > 32) throw Error(f + ": more than 32 batch axes");
    if (nbatch && !batch) throw Error(f + ": the batch shape is a null pointer");
    size_t items = 1;
    for (size_t i = 0; i < nbatch; ++i) {
        if (batch[i] == 0) return 0;  // an empty batch: nothing to do
        items *= batch[i];
        if (items >= ((size_t)1 << 31)) throw Error(f + ": more than 2^31 - 1 series in one call");
    }
    const bool comp = op == gft::SERIES_COMPOSE;
    SeriesArg ax = series_arg(fn, comp ? "f" : (corr ? "g" : (adj ? "gh" : "x")), x, xbs, nx, batch, nbatch, w, x0, rowst ? rowst[0] : 0);
    SeriesArg ay = series_arg(fn, comp || adj ? "g" : (binary ? "y" : "the seeds"), y, ybs, binary ? ny : 1, batch, nbatch, w, y0, rowst && binary ? rowst[1] : 0);
    SeriesArg ar = series_arg(fn, "the result", res, rbs, n, batch, nbatch, w, r0, rowst ? rowst[2] : 0);
    // the result's elements are distinct addresses: no zero stride, and sorted by stride every axis steps over the ones below it
    {
        struct Ax {
            size_t ext, st;
        } axes[35];
        int k = 0;
        if (w == 2) {  // the two planes are one more axis of the result
            if (ar.plane == 0) throw Error(f + ": the result has a zero plane stride: its lower and upper bounds overlap");
            axes[k++] = Ax{2, ar.plane};
        }
        for (size_t i = 0; i < nbatch; ++i) {
            if (batch[i] <= 1) continue;
            if (ar.st[i] == 0) throw Error(f + ": the result has a zero stride (batch axis " + std::to_string(i) + "): its series overlap");
            axes[k++] = Ax{batch[i], ar.st[i]};
        }
        if (r0 > 1) {  // rank 2: the rows of an item are one more axis of the result
            if (ar.rst == 0) throw Error(f + ": the result has a zero row stride: the rows of an item overlap");
            axes[k++] = Ax{r0, ar.rst};
        }
        if (n > 1) axes[k++] = Ax{n, 1};
        std::sort(axes, axes + k, [](const Ax& u, const Ax& v) { return u.st < v.st; });
        for (int i = 1; i < k; ++i)
            if (axes[i].st / axes[i - 1].ext < axes[i - 1].st)
                throw Error(f + ": the result's series overlap each other (its strides do not separate the rows)");
    }
    check_device_ptr(x, (f + ": " + ax.what).c_str());
    if (binary || y) check_device_ptr(y, (f + ": " + ay.what).c_str());
    check_device_ptr(res, (f + ": the result").c_str());
    // the result may be an input itself (the same view: every row is read before it is written); any other overlap is refused.
    // Judged by address ranges, so two interleaved views of one buffer count as overlapping.
    bool inplace = false;
    auto overlap = [&](const SeriesArg& a, bool same_ok) {
        if (a.p + a.span <= ar.p || ar.p + ar.span <= a.p) return;
        if (same_ok && series_same_view(a, ar, batch, nbatch)) {
            inplace = true;
            return;
        }
        throw Error(f + ": the result partially overlaps " + a.what + " (it may alias an operand only as the same view)");
    };
    overlap(ax, true);
    if (transposed) overlap(ay, false);  // corr's result may be g itself, compose_adj's gh; neither may be the second operand
    else if (binary) overlap(ay, true);
    else if (y) overlap(ay, false);
    // collapse the batch: unit axes go, axes contiguous with their inner neighbour on every operand merge
    gft::SeriesBatch g;
    g.nd = 0;
    g.items = (unsigned)items;
    g.inplace = inplace;
    const bool seeds = !binary && y;
    for (size_t i = 0; i < nbatch; ++i) {
        if (batch[i] == 1) continue;
        const size_t e = batch[i], sx = ax.st[i], sy = binary ? ay.st[i] : 0, ss = seeds ? ay.st[i] : 0, sr = ar.st[i];
        if (g.nd > 0) {
            const int p = g.nd - 1;
            // (merged extents stay below 2^31: items does)
            if (g.xs[p] == sx * e && g.ys[p] == sy * e && g.ss[p] == ss * e && g.rs[p] == sr * e) {
                g.ext[p] *= (unsigned)e;
                g.xs[p] = sx;
                g.ys[p] = sy;
                g.ss[p] = ss;
                g.rs[p] = sr;
                continue;
            }
        }
        // (the workspace copies add the series axis, and for intervals the plane axis, to these; pow at rank 2 the row axis too)
        const int most = gft::IMAXD - w - (d2 && op == gft::SERIES_POW ? 1 : 0);
        if (g.nd == most) throw Error(f + ": the batch has more than " + std::to_string(most) + " non-contiguous axes");
        g.ext[g.nd] = (unsigned)e;
        g.xs[g.nd] = sx;
        g.ys[g.nd] = sy;
        g.ss[g.nd] = ss;
        g.rs[g.nd] = sr;
        ++g.nd;
    }
    gft::SeriesPlanes pl;
    pl.w = w;
    pl.x = ax.plane;
    pl.y = binary ? ay.plane : 0;
    pl.s = seeds ? ay.plane : 0;
    pl.r = ar.plane;
    if (observe) {
        gft::Series2Dims d;
        d.nx0 = (unsigned)x0, d.nx1 = (unsigned)nx, d.ny0 = d.ny1 = 1, d.n0 = (unsigned)r0, d.n1 = (unsigned)n;
        d.xr = ax.rst, d.yr = 0, d.rr = ar.rst;
        // the factors depend on (op, k, len) only: computed once with the reference's rounding (k_factor_table's functor) and kept.
        // A table is written on the library's stream, where the kernel below runs: its first use is ordered behind it.
        Rc<Buf> tab;
        size_t tlen = 0;
        if (op == gft::SERIES_DERIVATIVE || op == gft::SERIES_COEFF) {
            tlen = d2 && var == 0 ? r0 : n;
            const int top = op == gft::SERIES_DERIVATIVE ? TAB_DERIV : TAB_COEFF;
            tab = w == 2 ? Ops<EIv>::cached_table(top, k, tlen) : Ops<EF64>::cached_table(top, k, tlen);
        }
        const hipStream_t cs = (hipStream_t)stream;
        join_caller_in(cs);
        gft::series_observe(R.stream, op, x, res, d, var, (unsigned)k, g, pl, tab ? tab->p : nullptr, tlen, d2 != nullptr);
        join_caller_out(cs);
        R.series_last = gft::SERIES_NONE;
        return 0;
    }
    if (d2) {  // one form; planned before the streams are joined (the planner may refuse)
        gft::Series2Dims d = *d2;
        d.xr = ax.rst, d.yr = ay.rst, d.rr = ar.rst;
        const hipStream_t cs = (hipStream_t)stream;
        if (op == gft::SERIES_POW) {
            Rc<Buf> ws = alloc_doubles(gft::series2_pow_workspace(g.items, d, w));  // (returned to the pool on exit, as below)
            join_caller_in(cs);
            gft::series2_pow(R.stream, x, e, res, d, g, ws->p, pl);
        } else {
            const gft::Series2Plan plan = gft::series2_plan(op, d, w);
            join_caller_in(cs);
            gft::series2_launch(R.stream, op, plan, x, y, res, d, g, var, pl);
        }
        join_caller_out(cs);
        R.series_last = gft::SERIES_FORM_B;
        return 0;
    }
    const int form = op == gft::SERIES_POW ? gft::SERIES_NONE : gft::series_plan(op, g.items, (unsigned)(transposed ? nx : n), R.series_force, w);
    const size_t wsn = gft::series_workspace(op, form, g.items, (unsigned)nx, (unsigned)n, w);
    Rc<Buf> ws;
    if (wsn) ws = alloc_doubles(wsn);  // (returned to the pool on exit: later launches follow these on the one stream)
    const hipStream_t cs = (hipStream_t)stream;
    join_caller_in(cs);
    int ran = form;
    if (op == gft::SERIES_POW) ran = gft::series_pow(R.stream, x, (unsigned)nx, e, res, (unsigned)n, g, ws->p, R.series_force, pl);
    else gft::series_launch(R.stream, op, form, x, (unsigned)nx, y, (unsigned)ny, res, (unsigned)n, g, wsn ? ws->p : nullptr, pl);
    join_caller_out(cs);
    R.series_last = ran;
    return 0;
}

}  // namespace

extern "C" {
int gft_series_mul(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny, double* res,
                   const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_MUL, "series_mul", x, xbs, nx, y, ybs, ny, res, rbs, n, batch, nbatch, stream); });
}
int gft_series_div(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny, double* res,
                   const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_DIV, "series_div", x, xbs, nx, y, ybs, ny, res, rbs, n, batch, nbatch, stream); });
}
int gft_series_exp(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs, double* res,
                   const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_EXP, "series_exp", x, xbs, nx, seed, sbs, 1, res, rbs, n, batch, nbatch, stream); });
}
int gft_series_log(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs, double* res,
                   const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_LOG, "series_log", x, xbs, nx, seed, sbs, 1, res, rbs, n, batch, nbatch, stream); });
}
int gft_series_compose(const double* f, const int64_t* fbs, size_t nf, const double* g, const int64_t* gbs, size_t ng, double* res,
                       const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_COMPOSE, "series_compose", f, fbs, nf, g, gbs, ng, res, rbs, n, batch, nbatch, stream); });
}
int gft_series_pow(const double* x, const int64_t* xbs, size_t nx, uint32_t e, double* res, const int64_t* rbs, size_t n,
                   const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_POW, "series_pow", x, xbs, nx, nullptr, nullptr, 1, res, rbs, n, batch, nbatch, stream, e); });
}
int gft_series_corr(const double* g, const int64_t* gbs, size_t ng, const double* y, const int64_t* ybs, size_t ny, double* res,
                    const int64_t* rbs, size_t m, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_CORR, "series_corr", g, gbs, ng, y, ybs, ny, res, rbs, m, batch, nbatch, stream); });
}
int gft_series_compose_adj(const double* gh, const int64_t* hbs, size_t n, const double* g, const int64_t* gbs, size_t ng, double* res,
                           const int64_t* rbs, size_t nf, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_COMPOSE_ADJ, "series_compose_adj", gh, hbs, n, g, gbs, ng, res, rbs, nf, batch, nbatch, stream); });
}
// Interval<F64>: the same calls on (lo, hi) planes; every stride array has nbatch + 1 entries, the plane stride first
int gfti_series_mul(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny, double* res,
                   const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_MUL, "interval series_mul", x, xbs, nx, y, ybs, ny, res, rbs, n, batch, nbatch, stream, 0, 2); });
}
int gfti_series_div(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny, double* res,
                   const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_DIV, "interval series_div", x, xbs, nx, y, ybs, ny, res, rbs, n, batch, nbatch, stream, 0, 2); });
}
int gfti_series_exp(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs, double* res,
                   const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_EXP, "interval series_exp", x, xbs, nx, seed, sbs, 1, res, rbs, n, batch, nbatch, stream, 0, 2); });
}
int gfti_series_log(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs, double* res,
                   const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_LOG, "interval series_log", x, xbs, nx, seed, sbs, 1, res, rbs, n, batch, nbatch, stream, 0, 2); });
}
int gfti_series_compose(const double* f, const int64_t* fbs, size_t nf, const double* g, const int64_t* gbs, size_t ng, double* res,
                       const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_COMPOSE, "interval series_compose", f, fbs, nf, g, gbs, ng, res, rbs, n, batch, nbatch, stream, 0, 2); });
}
int gfti_series_pow(const double* x, const int64_t* xbs, size_t nx, uint32_t e, double* res, const int64_t* rbs, size_t n,
                   const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series_call(gft::SERIES_POW, "interval series_pow", x, xbs, nx, nullptr, nullptr, 1, res, rbs, n, batch, nbatch, stream, e, 2); });
}
// rank 2: the last two axes are an item's coefficient array; xrs / yrs / rrs are the row strides
static int series2_call(int op, const char* fn, const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y,
                        const int64_t* ybs, int64_t yrs, size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1,
                        const size_t* batch, size_t nbatch, void* stream, uint32_t e = 0, int var = 0, int w = 1) {
    const size_t cap = gft::SERIES2_MAX_ELEMS + 1;  // (the limits are judged by series_call; this only keeps the narrowing below exact)
    gft::Series2Dims d;
    d.nx0 = (unsigned)std::min(nx0, cap), d.nx1 = (unsigned)std::min(nx1, cap), d.ny0 = (unsigned)std::min(ny0, cap), d.ny1 = (unsigned)std::min(ny1, cap);
    d.n0 = (unsigned)std::min(n0, cap), d.n1 = (unsigned)std::min(n1, cap);
    d.xr = d.yr = d.rr = 0;
    const int64_t rowst[3] = {xrs, yrs, rrs};
    return series_call(op, fn, x, xbs, d.nx1, y, ybs, d.ny1, res, rbs, d.n1, batch, nbatch, stream, e, w, &d, rowst, var);
}
int gft_series2_mul(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs, int64_t yrs,
                    size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                    void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_MUL, "series2_mul", x, xbs, xrs, nx0, nx1, y, ybs, yrs, ny0, ny1, res, rbs, rrs, n0, n1, batch, nbatch, stream); });
}
int gft_series2_div(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs, int64_t yrs,
                    size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                    void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_DIV, "series2_div", x, xbs, xrs, nx0, nx1, y, ybs, yrs, ny0, ny1, res, rbs, rrs, n0, n1, batch, nbatch, stream); });
}
int gft_series2_exp(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* seed, const int64_t* sbs, double* res,
                    const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_EXP, "series2_exp", x, xbs, xrs, nx0, nx1, seed, sbs, 0, 1, 1, res, rbs, rrs, n0, n1, batch, nbatch, stream); });
}
int gft_series2_log(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* seed, const int64_t* sbs, double* res,
                    const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_LOG, "series2_log", x, xbs, xrs, nx0, nx1, seed, sbs, 0, 1, 1, res, rbs, rrs, n0, n1, batch, nbatch, stream); });
}
int gft_series2_compose(const double* f, const int64_t* fbs, int64_t frs, size_t nf0, size_t nf1, const double* g, const int64_t* gbs, int64_t grs,
                        size_t ng0, size_t ng1, int var, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch,
                        size_t nbatch, void* stream) {
    return guard_int([&] {
        if (var != 0 && var != 1) throw Error("series2_compose: var = " + std::to_string(var) + " (the variable of f that g replaces is 0 or 1)");
        return series2_call(gft::SERIES_COMPOSE, "series2_compose", f, fbs, frs, nf0, nf1, g, gbs, grs, ng0, ng1, res, rbs, rrs, n0, n1, batch, nbatch, stream, 0, var);
    });
}
int gft_series2_pow(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, uint32_t e, double* res, const int64_t* rbs, int64_t rrs,
                    size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_POW, "series2_pow", x, xbs, xrs, nx0, nx1, nullptr, nullptr, 0, 1, 1, res, rbs, rrs, n0, n1, batch, nbatch, stream, e); });
}
// the transposed operations at rank 2 (f64 only): g / gh is the long side, the result the short one
int gft_series2_corr(const double* g, const int64_t* gbs, int64_t grs, size_t g0, size_t g1, const double* y, const int64_t* ybs, int64_t yrs,
                     size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t m0, size_t m1, const size_t* batch, size_t nbatch,
                     void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_CORR, "series2_corr", g, gbs, grs, g0, g1, y, ybs, yrs, ny0, ny1, res, rbs, rrs, m0, m1, batch, nbatch, stream); });
}
int gft_series2_compose_adj(const double* gh, const int64_t* hbs, int64_t hrs, size_t n0, size_t n1, const double* g, const int64_t* gbs, int64_t grs,
                            size_t ng0, size_t ng1, int var, double* res, const int64_t* rbs, int64_t rrs, size_t nf0, size_t nf1, const size_t* batch,
                            size_t nbatch, void* stream) {
    return guard_int([&] {
        if (var != 0 && var != 1) throw Error("series2_compose_adj: var = " + std::to_string(var) + " (the variable of f that g replaces is 0 or 1)");
        return series2_call(gft::SERIES_COMPOSE_ADJ, "series2_compose_adj", gh, hbs, hrs, n0, n1, g, gbs, grs, ng0, ng1, res, rbs, rrs, nf0, nf1, batch, nbatch, stream, 0, var);
    });
}
// Interval<F64> at rank 2: the same calls on (lo, hi) planes; every batch-stride array has nbatch + 1 entries, the plane stride first
int gfti_series2_mul(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs, int64_t yrs,
                     size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                     void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_MUL, "interval series2_mul", x, xbs, xrs, nx0, nx1, y, ybs, yrs, ny0, ny1, res, rbs, rrs, n0, n1, batch, nbatch, stream, 0, 0, 2); });
}
int gfti_series2_div(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs, int64_t yrs,
                     size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                     void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_DIV, "interval series2_div", x, xbs, xrs, nx0, nx1, y, ybs, yrs, ny0, ny1, res, rbs, rrs, n0, n1, batch, nbatch, stream, 0, 0, 2); });
}
int gfti_series2_exp(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* seed, const int64_t* sbs, double* res,
                     const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_EXP, "interval series2_exp", x, xbs, xrs, nx0, nx1, seed, sbs, 0, 1, 1, res, rbs, rrs, n0, n1, batch, nbatch, stream, 0, 0, 2); });
}
int gfti_series2_log(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* seed, const int64_t* sbs, double* res,
                     const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_LOG, "interval series2_log", x, xbs, xrs, nx0, nx1, seed, sbs, 0, 1, 1, res, rbs, rrs, n0, n1, batch, nbatch, stream, 0, 0, 2); });
}
int gfti_series2_compose(const double* f, const int64_t* fbs, int64_t frs, size_t nf0, size_t nf1, const double* g, const int64_t* gbs, int64_t grs,
                         size_t ng0, size_t ng1, int var, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch,
                         size_t nbatch, void* stream) {
    return guard_int([&] {
        if (var != 0 && var != 1) throw Error("interval series2_compose: var = " + std::to_string(var) + " (the variable of f that g replaces is 0 or 1)");
        return series2_call(gft::SERIES_COMPOSE, "interval series2_compose", f, fbs, frs, nf0, nf1, g, gbs, grs, ng0, ng1, res, rbs, rrs, n0, n1, batch, nbatch, stream, 0, var, 2);
    });
}
int gfti_series2_pow(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, uint32_t e, double* res, const int64_t* rbs, int64_t rrs,
                     size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {
    return guard_int([&] { return series2_call(gft::SERIES_POW, "interval series2_pow", x, xbs, xrs, nx0, nx1, nullptr, nullptr, 0, 1, 1, res, rbs, rrs, n0, n1, batch, nbatch, stream, e, 0, 2); });
}
// the observation ops: one operand, the order k (at rank 2 behind the variable), the result k shorter on that axis
#define GFT_SERIES_OBSERVE(PFX, WHAT, W)                                                                                                          \
    int PFX##series_derivative(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs, size_t n,               \
                               const size_t* batch, size_t nbatch, void* stream) {                                                                \
        return guard_int([&] { return series_call(gft::SERIES_DERIVATIVE, WHAT "series_derivative", x, xbs, nx, nullptr, nullptr, 1, res, rbs, n, \
                                                  batch, nbatch, stream, 0, W, nullptr, nullptr, 1, k); });                                       \
    }                                                                                                                                             \
    int PFX##series_taylor_expansion_of_coeff(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs,          \
                                              size_t n, const size_t* batch, size_t nbatch, void* stream) {                                       \
        return guard_int([&] { return series_call(gft::SERIES_COEFF, WHAT "series_taylor_expansion_of_coeff", x, xbs, nx, nullptr, nullptr, 1,    \
                                                  res, rbs, n, batch, nbatch, stream, 0, W, nullptr, nullptr, 1, k); });                          \
    }                                                                                                                                             \
    int PFX##series_shift_down(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs, size_t n,               \
                               const size_t* batch, size_t nbatch, void* stream) {                                                                \
        return guard_int([&] { return series_call(gft::SERIES_SHIFT_DOWN, WHAT "series_shift_down", x, xbs, nx, nullptr, nullptr, 1, res, rbs, n, \
                                                  batch, nbatch, stream, 0, W, nullptr, nullptr, 1, k); });                                       \
    }                                                                                                                                             \
    int PFX##series_evaluate_all_one(const double* x, const int64_t* xbs, size_t nx, double* res, const int64_t* rbs, const size_t* batch,        \
                                     size_t nbatch, void* stream) {                                                                               \
        return guard_int([&] { return series_call(gft::SERIES_EVAL_ONE, WHAT "series_evaluate_all_one", x, xbs, nx, nullptr, nullptr, 1, res,     \
                                                  rbs, 1, batch, nbatch, stream, 0, W, nullptr, nullptr, 1, 0); });                               \
    }                                                                                                                                             \
    int PFX##series2_derivative(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k, double* res,         \
                                const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {        \
        return guard_int([&] { return series2_observe(gft::SERIES_DERIVATIVE, WHAT "series2_derivative", x, xbs, xrs, nx0, nx1, var, k, res, rbs, \
                                                      rrs, n0, n1, batch, nbatch, stream, W); });                                                 \
    }                                                                                                                                             \
    int PFX##series2_taylor_expansion_of_coeff(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k,       \
                                               double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch,           \
                                               size_t nbatch, void* stream) {                                                                     \
        return guard_int([&] { return series2_observe(gft::SERIES_COEFF, WHAT "series2_taylor_expansion_of_coeff", x, xbs, xrs, nx0, nx1, var, k, \
                                                      res, rbs, rrs, n0, n1, batch, nbatch, stream, W); });                                       \
    }                                                                                                                                             \
    int PFX##series2_shift_down(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k, double* res,         \
                                const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream) {        \
        return guard_int([&] { return series2_observe(gft::SERIES_SHIFT_DOWN, WHAT "series2_shift_down", x, xbs, xrs, nx0, nx1, var, k, res, rbs, \
                                                      rrs, n0, n1, batch, nbatch, stream, W); });                                                 \
    }                                                                                                                                             \
    int PFX##series2_evaluate_all_one(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, double* res, const int64_t* rbs,  \
                                      const size_t* batch, size_t nbatch, void* stream) {                                                         \
        return guard_int([&] { return series2_observe(gft::SERIES_EVAL_ONE, WHAT "series2_evaluate_all_one", x, xbs, xrs, nx0, nx1, 0, 0, res,    \
                                                      rbs, 0, 1, 1, batch, nbatch, stream, W); });                                                \
    }
static int series2_observe(int op, const char* fn, const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k,
                           double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream, int w) {
    const size_t cap = gft::SERIES2_MAX_ELEMS + 1;  // (as in series2_call: the limits and the shapes are judged by series_call)
    gft::Series2Dims d;
    d.nx0 = (unsigned)std::min(nx0, cap), d.nx1 = (unsigned)std::min(nx1, cap), d.ny0 = d.ny1 = 1;
    d.n0 = (unsigned)std::min(n0, cap), d.n1 = (unsigned)std::min(n1, cap);
    d.xr = d.yr = d.rr = 0;
    const int64_t rowst[3] = {xrs, 0, rrs};
    return series_call(op, fn, x, xbs, d.nx1, nullptr, nullptr, 1, res, rbs, d.n1, batch, nbatch, stream, 0, w, &d, rowst, var, k);
}
GFT_SERIES_OBSERVE(gft_, "", 1)
GFT_SERIES_OBSERVE(gfti_, "interval ", 2)
#undef GFT_SERIES_OBSERVE
int gft_series_last_form(void) { return R.series_last; }
}
