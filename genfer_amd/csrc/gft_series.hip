// Batched univariate series kernels (gft_series.hpp): mul, div, exp, log, compose, pow of B independent truncated power series, in the
// reference's operation order per item, multiply and add rounded separately (-ffp-contract=off).  gfx950 only.
//
// Form A — one lane is one series.  A wave owns 64 consecutive items.  Their rows are loaded along the series axis
// (coalesced) into LDS at an ODD pitch in doubles, lane l's row at l * pitch + i: the 32 lanes of a ds_read_b64 half-wave
// then touch 32 distinct bank pairs (the argument of the interop tile's pitch of 65).  Each lane runs the scalar
// recurrence on its own row — every lane the same trip counts, since all items share (nx, ny, n), and the reference's order
// is literally the loop order — and the results return through LDS to coalesced stores.  Two arrays are resident per wave
// (mul: x and y, z overwrites y from the top down; div: y and the dividend, which r overwrites in place; exp / log: x and r),
// 64 * pitch * 8 bytes each.
//
// Form B — one workgroup is one series (mul; div is k_div_1d_wave / k_div_1d with an item index, gft_div2d.hip).  The row
// pair is staged in LDS; a thread owns the outputs k and n - 1 - k, together n + 1 terms, so every thread does the same work;
// the x address is wave-uniform and the y addresses are consecutive across lanes.  For exp / log, form B is form A's lane-per-series loop over a transposed global workspace
// ([n][B]: lane = item, so a wave's accesses coalesce); the transposes are interop copies with swapped strides.  That is the
// slow corner (B = 1 runs at the speed of the one-lane k_exp_1d / k_log_1d).
//
// compose (res = f(g), Horner) keeps the result row resident across its nf - 1 steps.  Form A: three arrays per wave (f, g, the
// result; a step runs in place from the top output down).  Form B: one workgroup per series for the whole loop, two result rows
// and g in LDS, every step mul form B's balanced product, steps separated by an LDS-only barrier.  pow has no kernel of its
// own beside the writer of the unit item: series_pow, the one driver of ranks 1, 2 and 3, walks the steps of series_pow_steps
// (gft_series_args.hpp) as SERIES_MUL launches of the call's rank on workspace items.
//
// corr (the transposed product, the adjoint of mul; f64 only) has mul's two forms with the roles turned round: form A's outputs
// overwrite g's row from the bottom up, form B's wave walks the offset k - i downwards in lock step.  compose_adj (the transposed
// Horner loop) is compose form B run backwards; it has no form A.
//
// Every function below is a template over the element functor: EF64 serves gft_series_*, EIv (Interval<F64>, the planes lo and hi
// a plane stride apart on every operand) gfti_series_*, EBig (BigFloat, the planes factor and exponent) gftb_series_*.  The entry
// points of gft_series.hpp pick the instantiation by the width and the element kind (by_elem).  EBig has the six arithmetic
// operations: the transposed kernels (corr, compose_adj) are not instantiated on it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <type_traits>

#include "gft_elem.hpp"
#include "gft_launch.hpp"
#include "gft_series.hpp"
#include "gft_series_kernels.hpp"

namespace gft {

namespace {

// ---- form A: LDS budget ---------------------------------------------------------------------------------------------------
// Two workgroups must fit the 160 KB of a CU: 80 KB each.  A wave holds 2 arrays of 64 * pitch doubles = 1 KB * pitch, so
// waves * pitch <= 80: 4 waves up to pitch 19 (n <= 19), 2 waves up to pitch 39 (n <= 39), 1 wave up to pitch 79 (n <= 79).
// Above 64 KB a kernel needs hipFuncAttributeMaxDynamicSharedMemorySize; if the runtime refuses it the budget is 64 KB
// (waves * pitch <= 64, n <= 63).
// compose holds three arrays, 1.5 KB * pitch a wave, so waves * pitch <= 53 (160 / 3): 4 waves up to pitch 13 (n <= 13), 2 waves up
// to pitch 25 (n <= 25), 1 wave up to pitch 53 (n <= 53, the largest n compose takes in form A); with 64 KB, 128 / 3: n <= 41.
// Interval<F64> (E::W = 2 planes per array: 2 KB * pitch a wave for two arrays): waves * pitch <= 40, so 4 waves up to pitch 9
// (n <= 9), 2 waves up to pitch 19 (n <= 19), 1 wave up to pitch 39 (n <= 39); with 64 KB, waves * pitch <= 32: n <= 31.
// Interval compose, 3 KB * pitch a wave: waves * pitch <= 26 (160 / 6), so 4 waves up to pitch 5 (n <= 5), 2 waves up to pitch 13
// (n <= 13), 1 wave up to pitch 25 (n <= 25); with 64 KB, 128 / 6: pitch <= 21, n <= 21.
constexpr unsigned SA_BUDGET_KB = 80;
constexpr unsigned SA_BUDGET_KB_PLAIN = 64;
// Form A needs enough items to fill waves: below this many items mul and div take form B, where a whole workgroup works on
// one series.  256 items = 4 waves of form A against 256 workgroups of form B: a reasoned value.  The sweep made afterwards
// (tools/bench_series.py --form A | B, profiles/r07/series_forms.txt; ms per call, the per-call floor is 0.037) says it is too
// low for the longer rows: (256, 16) A 0.037 B 0.037, (1024, 16) 0.038 / 0.037, (256, 48) 0.080 / 0.036, (1024, 48) 0.080 / 0.037,
// (4096, 64) 0.097 / 0.037 (div 0.100 / 0.046).  Form B was not timed above 4096 items, so the value stands.
// The interval kernels keep it: the two forms were not timed against each other for intervals.
constexpr unsigned SA_MIN_ITEMS = 256;

// the transposed operations exist on F64 (and are instantiated on Interval<F64>); BigFloat has none
template <class E>
constexpr bool HAS_TRANSPOSED = !std::is_same<E, EBig>::value;

// what the runtime granted, asked once per element type (the EIv and the EBig kernels are functions of their own)
template <class E>
struct Granted {
    static unsigned budget_kb;  // 0: not asked yet
    static int compose_b_big;   // -1: not asked yet
    static int compose_adj_big;
};
template <class E>
unsigned Granted<E>::budget_kb = 0;
template <class E>
int Granted<E>::compose_b_big = -1;
template <class E>
int Granted<E>::compose_adj_big = -1;

// largest odd pitch >= n, and the waves per workgroup the budget allows for it (0: the rows do not fit form A)
// (`arrays` of E::W planes of 64 * pitch doubles per wave: arrays * E::W * pitch / 2 KB)
template <class E>
unsigned form_a_waves(unsigned n, unsigned budget_kb, unsigned arrays = 2) {
    const unsigned pitch = n | 1;
    if (arrays * pitch * E::W > 2 * budget_kb) return 0;
    const unsigned w = 2 * budget_kb / (arrays * pitch * E::W);
    return w >= 4 ? 4 : (w >= 2 ? 2 : 1);
}
unsigned op_arrays(int op) { return op == SERIES_COMPOSE ? 3 : 2; }

template <class E>
unsigned budget_kb() {
    unsigned& kb = Granted<E>::budget_kb;
    if (kb) return kb;
    const void* ks[6] = {(const void*)k_series_mul_a<E>, (const void*)k_series_div_a<E>, (const void*)k_series_explog_a<E, false>,
                         (const void*)k_series_explog_a<E, true>, (const void*)k_series_compose_a<E>, nullptr};
    if constexpr (HAS_TRANSPOSED<E>) ks[5] = (const void*)k_series_corr_a<E>;
    kb = (unsigned)(grant_dynamic_lds(ks, HAS_TRANSPOSED<E> ? 6 : 5, SA_BUDGET_KB * 1024, SA_BUDGET_KB_PLAIN * 1024) / 1024);
    return kb;
}

// compose form B wants up to 96 KB (two result rows and g at n = 4096, or their two planes each at n = 2048); where the runtime
// grants only 64 KB, g stays in global memory
template <class E>
bool compose_b_big() {
    int& big = Granted<E>::compose_b_big;
    if (big < 0) {
        big = hipFuncSetAttribute((const void*)k_series_compose_b<E, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  3 * E::W * series_limit(1, E::W) * sizeof(double)) == hipSuccess;
        if (!big) (void)hipGetLastError();
    }
    return big != 0;
}

// compose_adj's request is the same: two rows of gh and g
template <class E>
bool compose_adj_big() {
    int& big = Granted<E>::compose_adj_big;
    if (big < 0) {
        big = hipFuncSetAttribute((const void*)k_series_compose_adj_b<E, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  3 * E::W * series_limit(1, E::W) * sizeof(double)) == hipSuccess;
        if (!big) (void)hipGetLastError();
    }
    return big != 0;
}

// the batch of `g` over workspace rows: C-contiguous rows xp / yp / rp doubles apart (0: one row for every item; rp == 0 keeps
// the result's own strides)
SeriesBatch ws_batch(const SeriesBatch& g, size_t xp, size_t yp, size_t rp) {
    SeriesBatch w = g;
    w.inplace = 0;
    size_t cs = 1;
    for (int a = g.nd - 1; a >= 0; --a) {
        w.xs[a] = cs * xp;
        w.ys[a] = cs * yp;
        w.ss[a] = 0;
        if (rp) w.rs[a] = cs * rp;
        cs *= g.ext[a];
    }
    return w;
}

// a copy between the caller's rows (batch strides `bs`, planes `plane` apart) and a workspace [E::W][...] whose planes are `wplane`
// apart, item stride `wi` and coefficient stride `wc`; `in`: towards the workspace
template <class E>
void ws_copy(hipStream_t st, const double* src, double* dst, const SeriesBatch& g, const size_t* bs, size_t plane, unsigned len,
             size_t wplane, size_t wi, size_t wc, bool in) {
    CopyGeom c;
    int k = 0;
    if (E::W > 1) {
        c.ext[k] = E::W;
        c.ss[k] = in ? plane : wplane;
        c.ds[k] = in ? wplane : plane;
        ++k;
    }
    size_t cs = wi;
    for (int a = g.nd - 1; a >= 0; --a) {
        c.ext[k + a] = g.ext[a];
        c.ss[k + a] = in ? bs[a] : cs;
        c.ds[k + a] = in ? cs : bs[a];
        cs *= g.ext[a];
    }
    k += g.nd;
    c.ext[k] = len;
    c.ss[k] = in ? 1 : wc;
    c.ds[k] = in ? wc : 1;
    c.nd = k + 1;
    interop_copy(st, src, dst, c);
}

template <class E>
int plan(int op, unsigned items, unsigned n, int force) {
    if (op == SERIES_COMPOSE_ADJ) return SERIES_FORM_B;  // its one form
    const bool fits = form_a_waves<E>(n, budget_kb<E>(), op_arrays(op)) != 0;
    if (!fits || force == SERIES_FORM_B) return SERIES_FORM_B;
    if (force == SERIES_FORM_A) return SERIES_FORM_A;
    if (op == SERIES_EXP || op == SERIES_LOG) return SERIES_FORM_A;  // form B of these is the slow corner whatever the batch
    return items >= SA_MIN_ITEMS ? SERIES_FORM_A : SERIES_FORM_B;
}

template <class E>
void launch(hipStream_t st, int op, int form, const double* x, unsigned nx, const double* y, unsigned ny, double* res, unsigned n,
            const SeriesBatch& g, double* ws, const SeriesPlanes& pl) {
    if (g.items == 0) return;
    if (form == SERIES_FORM_A) {
        const unsigned rows = op == SERIES_CORR ? nx : n;  // the longest row a lane holds (corr: g, its result is shorter)
        const unsigned pitch = rows | 1;
        const unsigned arrays = op_arrays(op);
        unsigned waves = form_a_waves<E>(rows, budget_kb<E>(), arrays);
        if (waves == 0) throw std::runtime_error("series: rows of " + std::to_string(rows) + " coefficients do not fit form A");
        const unsigned wave_items = (g.items + 63) / 64;
        waves = std::min(waves, wave_items);
        if (waves == 3) waves = 2;
        unsigned lg = 0;  // lanes per row while staging: the smallest power of two >= n, at most 64
        while (lg < 6 && (1u << lg) < rows) ++lg;
        const dim3 grid((wave_items + waves - 1) / waves), block(64 * waves);
        const size_t lds = (size_t)waves * arrays * E::W * 64 * pitch * sizeof(double);
        switch (op) {
            case SERIES_MUL: GFT_LAUNCH(k_series_mul_a<E>, grid, block, lds, st, x, pl.x, nx, y, pl.y, ny, res, pl.r, n, pitch, lg, g); break;
            case SERIES_DIV: GFT_LAUNCH(k_series_div_a<E>, grid, block, lds, st, x, pl.x, nx, y, pl.y, ny, res, pl.r, n, pitch, lg, g); break;
            case SERIES_COMPOSE: GFT_LAUNCH(k_series_compose_a<E>, grid, block, lds, st, x, pl.x, nx, y, pl.y, ny, res, pl.r, n, pitch, lg, g); break;
            case SERIES_CORR:
                if constexpr (HAS_TRANSPOSED<E>) GFT_LAUNCH(k_series_corr_a<E>, grid, block, lds, st, x, pl.x, nx, y, pl.y, ny, res, pl.r, n, pitch, lg, g);
                else throw std::runtime_error("series: no transposed product on this element");
                break;
            case SERIES_COMPOSE_ADJ: throw std::runtime_error("series: compose_adj has no form A");
            case SERIES_EXP: GFT_LAUNCH((k_series_explog_a<E, false>), grid, block, lds, st, x, pl.x, nx, y, pl.s, res, pl.r, n, pitch, lg, g); break;
            default: GFT_LAUNCH((k_series_explog_a<E, true>), grid, block, lds, st, x, pl.x, nx, y, pl.s, res, pl.r, n, pitch, lg, g); break;
        }
        return;
    }
    if (op == SERIES_MUL) {
        // few series: 64 outputs pairs per workgroup, so that one long series spreads over the CUs ((1, 4096): 32 workgroups);
        // many series (or a result in place, which one workgroup must own): 256 threads, fewer copies of the row pair
        const unsigned half = (n + 1) / 2;
        const bool spread = !g.inplace && g.items < SA_MIN_ITEMS;
        const unsigned threads = spread ? 64u : std::min(256u, (half + 63) / 64 * 64);
        const unsigned shares = g.inplace ? 1u : (half + threads - 1) / threads;
        GFT_LAUNCH(k_series_mul_b<E>, dim3(g.items, shares), dim3(threads), (size_t)E::W * ((size_t)nx + ny) * sizeof(double), st, x, pl.x, nx,
                   y, pl.y, ny, res, pl.r, n, g);
        return;
    }
    if constexpr (!HAS_TRANSPOSED<E>) {
        if (op == SERIES_CORR || op == SERIES_COMPOSE_ADJ) throw std::runtime_error("series: no transposed operation on this element");
    } else {
        if (op == SERIES_CORR) {  // mul's geometry over the m = n outputs
            const unsigned half = (n + 1) / 2;
            const bool spread = !g.inplace && g.items < SA_MIN_ITEMS;
            const unsigned threads = spread ? 64u : std::min(256u, (half + 63) / 64 * 64);
            const unsigned shares = g.inplace ? 1u : (half + threads - 1) / threads;
            GFT_LAUNCH(k_series_corr_b<E>, dim3(g.items, shares), dim3(threads), (size_t)E::W * ((size_t)nx + ny) * sizeof(double), st, x, pl.x, nx,
                       y, pl.y, ny, res, pl.r, n, g);
            return;
        }
        if (op == SERIES_COMPOSE_ADJ) {  // x = gh (nx = the order n), y = g, n = nf outputs
            const unsigned full = (n - 1) * (ny - 1) + 1, l0 = std::min(full, nx);
            const unsigned threads = std::min(256u, ((l0 + 1) / 2 + 63) / 64 * 64);
            const size_t rows = (size_t)2 * E::W * l0 * sizeof(double), all = rows + (size_t)E::W * ny * sizeof(double);
            if (all <= 64 * 1024 || compose_adj_big<E>())
                GFT_LAUNCH((k_series_compose_adj_b<E, true>), dim3(g.items), dim3(threads), all, st, x, pl.x, nx, y, pl.y, ny, res, pl.r, n, g);
            else
                GFT_LAUNCH((k_series_compose_adj_b<E, false>), dim3(g.items), dim3(threads), rows, st, x, pl.x, nx, y, pl.y, ny, res, pl.r, n, g);
            return;
        }
    }
    if (op == SERIES_COMPOSE) {
        const unsigned threads = std::min(256u, ((n + 1) / 2 + 63) / 64 * 64);
        const size_t rows = (size_t)2 * E::W * n * sizeof(double), all = rows + (size_t)E::W * ny * sizeof(double);
        if (all <= 64 * 1024 || compose_b_big<E>())
            GFT_LAUNCH((k_series_compose_b<E, true>), dim3(g.items), dim3(threads), all, st, x, pl.x, nx, y, pl.y, ny, res, pl.r, n, g);
        else
            GFT_LAUNCH((k_series_compose_b<E, false>), dim3(g.items), dim3(threads), rows, st, x, pl.x, nx, y, pl.y, ny, res, pl.r, n, g);
        return;
    }
    if (op == SERIES_DIV) {
        series_div_rows(st, x, nx, y, ny, res, n, g, pl);
        return;
    }
    // exp / log: x -> xT [plane][nx][items], the lane-per-item loop, rT [plane][n][items] -> res
    double* xT = ws;
    double* rT = ws + (size_t)E::W * ((size_t)g.items * nx);
    ws_copy<E>(st, x, xT, g, g.xs, pl.x, nx, (size_t)nx * g.items, 1, g.items, true);
    const dim3 grid((g.items + 63) / 64), block(64);
    if (op == SERIES_EXP) GFT_LAUNCH((k_series_explog_ws<E, false>), grid, block, 0, st, xT, nx, y, pl.s, rT, n, g);
    else GFT_LAUNCH((k_series_explog_ws<E, true>), grid, block, 0, st, xT, nx, y, pl.s, rT, n, g);
    ws_copy<E>(st, rT, res, g, g.rs, pl.r, n, (size_t)n * g.items, 1, g.items, false);
}

// the unit item of pow: 1.0 at [0, 0, 0] and +0.0 elsewhere, through the result's three strides -- its first factor (one item of one
// coefficient) and the whole result of e == 0 (an interval item: [1,1] and [0,0], both planes `plane` apart); a lower rank has
// leading lengths of 1
template <class E>
__global__ __launch_bounds__(256) void k_series_unit(double* res, size_t plane, size_t s0, size_t s1, size_t s2, unsigned n0, unsigned n1,
                                                     unsigned n2, SeriesBatch b) {
    const SeriesOff o = series_offsets(b, blockIdx.x);
    const unsigned n12 = n1 * n2;
    for (unsigned idx = threadIdx.x; idx < n0 * n12; idx += blockDim.x) {
        const unsigned k0 = idx / n12, r = idx - k0 * n12, k1 = r / n2, k2 = r - k1 * n2;
        E::st(res, plane, o.r + (size_t)k0 * s0 + (size_t)k1 * s1 + (size_t)k2 * s2, idx == 0 ? E::one() : E::zero());
    }
}

// pow at every rank: the steps of series_pow_steps on workspace items, every product the rank's own SERIES_MUL launch
template <class E>
int pow_steps(hipStream_t st, int rank, const double* x, unsigned e, double* res, const SeriesItem& it, const SeriesBatch& g, double* ws, int force,
              const SeriesPlanes& pl) {
    int form = rank == 1 ? SERIES_NONE : SERIES_FORM_B;
    if (std::is_same<E, EBig>::value && rank != 1) throw std::runtime_error("series: BigFloat pow exists at rank 1 only");  // (series_shapes refuses it)
    if (g.items == 0) return form;
    const unsigned* n = it.n;
    const unsigned N = n[0] * n[1] * n[2];
    if (e == 0) {
        GFT_LAUNCH(k_series_unit<E>, dim3(g.items), dim3(series_threads(N)), 0, st, res, pl.r, it.rs[0], it.rs[1], it.rs[2], n[0], n[1], n[2], g);
        return form;
    }
    // three workspace arrays of items * N elements each, whatever the compact shape of the items in it, and the unit item; plane-major:
    // the upper bounds of everything in the workspace lie `wp` doubles behind the lower ones.  wp is odd where items * N is even, so
    // the planes share no 16-byte alignment -- which costs nothing: every global access of the series kernels is one double wide
    // (checked in the gfx950 code of gft_series*.hip and gft_div2d.hip: no 128-bit global load or store), and the interop copy
    // takes two at a time only in its dense form and only between 16-byte aligned pointers.
    const size_t arr = (size_t)g.items * N, wp = 3 * arr + 1;
    double* const slot[5] = {ws + 3 * arr, ws, ws + arr, ws + 2 * arr, res};  // by SeriesPowSlot
    SeriesBatch one;
    one.nd = 0;
    one.items = 1;
    GFT_LAUNCH(k_series_unit<E>, dim3(1), dim3(64), 0, st, slot[POW_UNIT], wp, (size_t)1, (size_t)1, (size_t)1, 1u, 1u, 1u, one);
    {
        // the operand, read once through its strides into compact items of nx: the planes, the batch, the series axes of the rank
        CopyGeom c;
        int k = 0;
        if (E::W == 2) c.ext[k] = 2, c.ss[k] = pl.x, c.ds[k] = wp, ++k;
        size_t cs = (size_t)it.nx[0] * it.nx[1] * it.nx[2];
        for (int a = g.nd - 1; a >= 0; --a) {
            c.ext[k + a] = g.ext[a];
            c.ss[k + a] = g.xs[a];
            c.ds[k + a] = cs;
            cs *= g.ext[a];
        }
        k += g.nd;
        const size_t xc[3] = {(size_t)it.nx[1] * it.nx[2], it.nx[2], 1};
        for (int a = 3 - rank; a < 3; ++a) c.ext[k] = it.nx[a], c.ss[k] = it.xs[a], c.ds[k] = xc[a], ++k;
        c.nd = k;
        interop_copy(st, x, slot[POW_WS0], c);
    }
    const SeriesPowSteps steps = series_pow_steps(e, it.nx, n);
    for (int i = 0; i < steps.count; ++i) {
        const SeriesPowStep& s = steps.step[i];
        // a (stored shape sa; maybe the one unit item) * b (sb), compact workspace items, into `out`: compact at L, or (last) the
        // caller's result at all of n
        const unsigned *sa = s.sa, *sb = s.sb, *lo = s.last ? n : s.L;
        const size_t lc[3] = {(size_t)s.L[1] * s.L[2], s.L[2], 1}, *os = s.last ? it.rs : lc;
        const double *a = slot[s.a], *b = slot[s.b];
        double* out = slot[s.out];
        const SeriesBatch w = ws_batch(g, s.a == POW_UNIT ? 0 : (size_t)sa[0] * sa[1] * sa[2], (size_t)sb[0] * sb[1] * sb[2], s.last ? 0 : lc[0] * s.L[0]);
        SeriesPlanes wpl;
        wpl.w = E::W, wpl.elem = pl.elem;
        if (E::W == 2) wpl.x = wpl.y = wp, wpl.r = s.last ? pl.r : wp;  // (one plane: the strides stay 0)
        if (rank == 1) {
            form = plan<E>(SERIES_MUL, g.items, lo[2], force);
            launch<E>(st, SERIES_MUL, form, a, sa[2], b, sb[2], out, lo[2], w, nullptr, wpl);
        } else if (rank == 2) {
            const Series2Dims m{sa[1], sa[2], sb[1], sb[2], lo[1], lo[2], sa[2], sb[2], os[1]};
            series2_launch(st, SERIES_MUL, series2_plan(SERIES_MUL, m, E::W), a, b, out, m, w, 0, wpl);
        } else {
            const Series3Dims m = series3_product_dims(sa, sb, lo, os);
            series3_launch(st, SERIES_MUL, series3_plan(SERIES_MUL, m, E::W), a, b, out, m, w, wpl);
        }
    }
    return form;
}

// the instantiation of a call: BigFloat by the element kind, else by the width
template <class F>
auto by_elem(int w, int elem, F&& f) {
    if (elem == SERIES_ELEM_BIGFLOAT) return f(EBig());
    if (w == 2) return f(EIv());
    return f(EF64());
}

}  // namespace

int series_plan(int op, unsigned items, unsigned n, int force, int w, int elem) {
    return by_elem(w, elem, [&](auto e) { return plan<decltype(e)>(op, items, n, force); });
}

size_t series_workspace(int op, int form, unsigned items, unsigned nx, unsigned n, int w) {
    if (form != SERIES_FORM_B || (op != SERIES_EXP && op != SERIES_LOG)) return 0;
    return (size_t)w * items * ((size_t)nx + n);
}

void series_launch(hipStream_t st, int op, int form, const double* x, unsigned nx, const double* y, unsigned ny, double* res,
                   unsigned n, const SeriesBatch& g, double* ws, const SeriesPlanes& pl) {
    by_elem(pl.w, pl.elem, [&](auto e) { launch<decltype(e)>(st, op, form, x, nx, y, ny, res, n, g, ws, pl); });
}

size_t series_pow_workspace(unsigned items, const unsigned* n, int w) { return (size_t)w * (3 * (size_t)items * n[0] * n[1] * n[2] + 1); }

int series_pow(hipStream_t st, int rank, const double* x, unsigned e, double* res, const SeriesItem& it, const SeriesBatch& g, double* ws,
               int force, const SeriesPlanes& pl) {
    return by_elem(pl.w, pl.elem, [&](auto el) { return pow_steps<decltype(el)>(st, rank, x, e, res, it, g, ws, force, pl); });
}

}  // namespace gft
