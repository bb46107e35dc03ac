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
// own: series_pow plans a sequence of mul launches on workspace rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>

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
constexpr unsigned SA_BUDGET_KB = 80;
constexpr unsigned SA_BUDGET_KB_PLAIN = 64;
// Form A needs enough items to fill waves: below this many items mul and div take form B, where a whole workgroup works on
// one series.  256 items = 4 waves of form A against 256 workgroups of form B: a reasoned value.  The sweep made afterwards
// (tools/bench_series.py --form A | B, profiles/r07/series_forms.txt; ms per call, the per-call floor is 0.037) says it is too
// low for the longer rows: (256, 16) A 0.037 B 0.037, (1024, 16) 0.038 / 0.037, (256, 48) 0.080 / 0.036, (1024, 48) 0.080 / 0.037,
// (4096, 64) 0.097 / 0.037 (div 0.100 / 0.046).  Form B was not timed above 4096 items, so the value stands.
constexpr unsigned SA_MIN_ITEMS = 256;

unsigned g_budget_kb = 0;  // 0: not asked yet

typedef EF64 E;

// largest odd pitch >= n, and the waves per workgroup the budget allows for it (0: the rows do not fit form A)
// (`arrays` of 64 * pitch doubles per wave: arrays * pitch / 2 KB)
unsigned form_a_waves(unsigned n, unsigned budget_kb, unsigned arrays = 2) {
    const unsigned pitch = n | 1;
    if (arrays * pitch * E::W > 2 * budget_kb) return 0;
    const unsigned w = 2 * budget_kb / (arrays * pitch * E::W);
    return w >= 4 ? 4 : (w >= 2 ? 2 : 1);
}
unsigned op_arrays(int op) { return op == SERIES_COMPOSE ? 3 : 2; }

unsigned budget_kb() {
    if (g_budget_kb) return g_budget_kb;
    const void* ks[] = {(const void*)k_series_mul_a<E>, (const void*)k_series_div_a<E>, (const void*)k_series_explog_a<E, false>,
                        (const void*)k_series_explog_a<E, true>, (const void*)k_series_compose_a<E>};
    g_budget_kb = SA_BUDGET_KB;
    for (const void* k : ks)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, SA_BUDGET_KB * 1024) != hipSuccess) {
            (void)hipGetLastError();  // no stale error for the caller's next HIP call
            g_budget_kb = SA_BUDGET_KB_PLAIN;
            break;
        }
    return g_budget_kb;
}

// compose form B wants up to 96 KB (two result rows and g at n = 4096); where the runtime grants only 64 KB, g stays in global memory
int g_compose_b_big = -1;  // -1: not asked yet
bool compose_b_big() {
    if (g_compose_b_big < 0) {
        g_compose_b_big = hipFuncSetAttribute((const void*)k_series_compose_b<E, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              3 * E::W * SERIES_MAX_N * sizeof(double)) == hipSuccess;
        if (!g_compose_b_big) (void)hipGetLastError();
    }
    return g_compose_b_big != 0;
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

}  // namespace

int series_plan(int op, unsigned items, unsigned n, int force) {
    const bool fits = form_a_waves(n, budget_kb(), op_arrays(op)) != 0;
    if (!fits || force == SERIES_FORM_B) return SERIES_FORM_B;
    if (force == SERIES_FORM_A) return SERIES_FORM_A;
    if (op == SERIES_EXP || op == SERIES_LOG) return SERIES_FORM_A;  // form B of these is the slow corner whatever the batch
    return items >= SA_MIN_ITEMS ? SERIES_FORM_A : SERIES_FORM_B;
}

size_t series_workspace(int op, int form, unsigned items, unsigned nx, unsigned n) {
    if (op == SERIES_POW) return (size_t)E::W * (3 * (size_t)items * n + 1);
    if (form != SERIES_FORM_B || (op != SERIES_EXP && op != SERIES_LOG)) return 0;
    return (size_t)E::W * items * ((size_t)nx + n);
}

void series_launch(hipStream_t st, int op, int form, const double* x, unsigned nx, const double* y, unsigned ny, double* res,
                   unsigned n, const SeriesBatch& g, double* ws) {
    if (g.items == 0) return;
    if (form == SERIES_FORM_A) {
        const unsigned pitch = n | 1;
        const unsigned arrays = op_arrays(op);
        unsigned waves = form_a_waves(n, budget_kb(), arrays);
        if (waves == 0) throw std::runtime_error("series: rows of " + std::to_string(n) + " coefficients do not fit form A");
        const unsigned wave_items = (g.items + 63) / 64;
        waves = std::min(waves, wave_items);
        if (waves == 3) waves = 2;
        unsigned lg = 0;  // lanes per row while staging: the smallest power of two >= n, at most 64
        while (lg < 6 && (1u << lg) < n) ++lg;
        const dim3 grid((wave_items + waves - 1) / waves), block(64 * waves);
        const size_t lds = (size_t)waves * arrays * E::W * 64 * pitch * sizeof(double);
        switch (op) {
            case SERIES_MUL: GFT_LAUNCH(k_series_mul_a<E>, grid, block, lds, st, x, (size_t)0, nx, y, (size_t)0, ny, res, (size_t)0, n, pitch, lg, g); break;
            case SERIES_DIV: GFT_LAUNCH(k_series_div_a<E>, grid, block, lds, st, x, (size_t)0, nx, y, (size_t)0, ny, res, (size_t)0, n, pitch, lg, g); break;
            case SERIES_COMPOSE: GFT_LAUNCH(k_series_compose_a<E>, grid, block, lds, st, x, (size_t)0, nx, y, (size_t)0, ny, res, (size_t)0, n, pitch, lg, g); break;
            case SERIES_EXP: GFT_LAUNCH((k_series_explog_a<E, false>), grid, block, lds, st, x, (size_t)0, nx, y, (size_t)0, res, (size_t)0, n, pitch, lg, g); break;
            default: GFT_LAUNCH((k_series_explog_a<E, true>), grid, block, lds, st, x, (size_t)0, nx, y, (size_t)0, res, (size_t)0, n, pitch, lg, g); break;
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
        GFT_LAUNCH(k_series_mul_b<E>, dim3(g.items, shares), dim3(threads), (size_t)E::W * ((size_t)nx + ny) * sizeof(double), st, x, (size_t)0, nx,
                   y, (size_t)0, ny, res, (size_t)0, n, g);
        return;
    }
    if (op == SERIES_COMPOSE) {
        const unsigned threads = std::min(256u, ((n + 1) / 2 + 63) / 64 * 64);
        const size_t rows = (size_t)2 * E::W * n * sizeof(double), all = rows + (size_t)E::W * ny * sizeof(double);
        if (all <= 64 * 1024 || compose_b_big())
            GFT_LAUNCH((k_series_compose_b<E, true>), dim3(g.items), dim3(threads), all, st, x, (size_t)0, nx, y, (size_t)0, ny, res, (size_t)0, n, g);
        else
            GFT_LAUNCH((k_series_compose_b<E, false>), dim3(g.items), dim3(threads), rows, st, x, (size_t)0, nx, y, (size_t)0, ny, res, (size_t)0, n, g);
        return;
    }
    if (op == SERIES_DIV) {
        series_div_rows(st, x, nx, y, ny, res, n, g);
        return;
    }
    // exp / log: x -> xT, the lane-per-item loop, rT -> res
    double* xT = ws;
    double* rT = ws + (size_t)E::W * ((size_t)g.items * nx);
    CopyGeom in, out;
    size_t cs = 1;  // C stride of the batch axis inside an [..][items] workspace
    in.nd = out.nd = g.nd + 1;
    for (int a = g.nd - 1; a >= 0; --a) {
        in.ext[a] = out.ext[a] = g.ext[a];
        in.ss[a] = g.xs[a];
        in.ds[a] = cs;
        out.ss[a] = cs;
        out.ds[a] = g.rs[a];
        cs *= g.ext[a];
    }
    in.ext[g.nd] = nx;
    in.ss[g.nd] = 1;
    in.ds[g.nd] = g.items;
    out.ext[g.nd] = n;
    out.ss[g.nd] = g.items;
    out.ds[g.nd] = 1;
    interop_copy(st, x, xT, in);
    const dim3 grid((g.items + 63) / 64), block(64);
    if (op == SERIES_EXP) GFT_LAUNCH((k_series_explog_ws<E, false>), grid, block, 0, st, xT, nx, y, (size_t)0, rT, n, g);
    else GFT_LAUNCH((k_series_explog_ws<E, true>), grid, block, 0, st, xT, nx, y, (size_t)0, rT, n, g);
    interop_copy(st, rT, res, out);
}

int series_pow(hipStream_t st, const double* x, unsigned nx, unsigned e, double* res, unsigned n, const SeriesBatch& g, double* ws,
               int force) {
    if (g.items == 0) return SERIES_NONE;
    if (e == 0) {
        GFT_LAUNCH(k_series_unit_rows<E>, dim3(g.items), dim3(std::min(256u, (n + 63) / 64 * 64)), 0, st, res, (size_t)0, n, g);
        return SERIES_NONE;
    }
    const size_t rows = (size_t)E::W * g.items * n;
    double* spare[2] = {ws + rows, ws + 2 * rows};
    int nspare = 2;
    double* unit = ws + 3 * rows;
    SeriesBatch one_row;
    one_row.nd = 0;
    one_row.items = 1;
    GFT_LAUNCH(k_series_unit_rows<E>, dim3(1), dim3(64), 0, st, unit, (size_t)0, 1u, one_row);
    // the operand, read once through its strides: base = x as rows of nx
    double* base = ws;
    unsigned lb = nx;
    {
        CopyGeom in;
        size_t cs = 1;
        in.nd = g.nd + 1;
        for (int a = g.nd - 1; a >= 0; --a) {
            in.ext[a] = g.ext[a];
            in.ss[a] = g.xs[a];
            in.ds[a] = cs * nx;
            cs *= g.ext[a];
        }
        in.ext[g.nd] = nx;
        in.ss[g.nd] = in.ds[g.nd] = 1;
        interop_copy(st, x, base, in);
    }
    double* acc = unit;  // res of mt:441: [1.0] for every item until the first product
    unsigned la = 1;
    int form = SERIES_NONE;
    auto product = [&](const double* a, unsigned na, size_t ap, const double* b, unsigned nb, double* out, unsigned len, bool last) {
        form = series_plan(SERIES_MUL, g.items, len, force);
        series_launch(st, SERIES_MUL, form, a, na, b, nb, out, len, ws_batch(g, ap, nb, last ? 0 : len), nullptr);
    };
    while (e > 0) {
        if (e & 1) {
            const bool last = (e >> 1) == 0;
            const unsigned len = std::min(la + lb - 1, n);
            double* out = last ? res : spare[--nspare];
            product(acc, la, acc == unit ? 0 : la, base, lb, out, last ? n : len, last);
            if (acc != unit) spare[nspare++] = acc;
            acc = out;
            la = len;
        }
        e >>= 1;
        if (e > 0) {
            const unsigned len = std::min(2 * lb - 1, n);
            double* out = spare[--nspare];
            product(base, lb, lb, base, lb, out, len, false);
            spare[nspare++] = base;
            base = out;
            lb = len;
        }
    }
    return form;
}

}  // namespace gft
