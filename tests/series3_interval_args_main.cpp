// Rank-3 interval calls (w == 2) in the host-side argument layer (genfer_amd/csrc/gft_series_args.hpp) on their own: no HIP, no device.
// A self-checking program (tests/test_interval_series3_cpu.py builds and runs it, under the address and undefined-behaviour
// sanitizers where they are available; exit status 0 and a last line "ok <n> checks" when all holds):
//   * the six operations are admitted with w == 2, the limit is 2048 with its text, f64 keeps 4096;
//   * the plane stride leads the batch-stride array of every operand, and a null array means planes back to back;
//   * the result's planes join the distinct-address proof and the overlap proof; "the same view" includes the plane stride;
//   * pow's cap on non-contiguous batch axes is one lower than at f64;
//   * an operation rank 3 lacks keeps its text for w == 1 and w == 2;
//   * the device-free sizes of the div / exp / log scratch (series3_sizes) at the shapes the GPU tests run.
#include <cstdio>
#include <string>

#include "../genfer_amd/csrc/gft_series_args.hpp"

static double buffer[1 << 17];
static long checks = 0, failures = 0;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++checks;                                                                     \
        if (!(cond)) {                                                                \
            if (++failures <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                             \
    } while (0)

static gft::SeriesView view(size_t off, const unsigned* s, const int64_t* bs = nullptr) {
    gft::SeriesView v;
    v.p = buffer + off, v.bs = bs;
    v.len[0] = s[0], v.len[1] = s[1], v.len[2] = s[2];
    v.st[0] = (int64_t)(s[1] * s[2]), v.st[1] = (int64_t)s[2];
    return v;
}

static std::string verdict(const gft::SeriesCall& c, gft::SeriesArgs* out = nullptr) {
    try {
        gft::SeriesArgs a;
        gft::series_args(c, a, [](const double*, const char*) {});
        if (out) *out = a;
        return "";
    } catch (const std::exception& e) {
        return e.what();
    }
}

static void expect(const gft::SeriesCall& c, const std::string& want) {
    const std::string got = verdict(c);
    ++checks;
    if (got != want) {
        if (++failures <= 20) std::printf("FAILED: want \"%s\"\n        got  \"%s\"\n", want.c_str(), got.c_str());
    }
}

static const char* NAMES[6] = {"interval series3_mul", "interval series3_div", "interval series3_exp", "interval series3_log",
                               "interval series3_compose", "interval series3_pow"};

// a call of operation `op` on items of n, x at 0, y at 16384, the result at 32768 (planes back to back unless bs says otherwise)
static gft::SeriesCall call(int op, const unsigned* nx, const unsigned* n, const size_t* batch, size_t nbatch, int w = 2) {
    gft::SeriesCall c;
    c.op = op, c.fn = w == 2 ? NAMES[op] : NAMES[op] + 9, c.w = w, c.rank = 3, c.batch = batch, c.nbatch = nbatch, c.e = 5;
    c.x = view(0, nx), c.r = view(32768, n);
    const unsigned one[3] = {1, 1, 1};
    if (op == gft::SERIES_MUL || op == gft::SERIES_DIV || op == gft::SERIES_COMPOSE) c.y = view(16384, nx);
    else if (op != gft::SERIES_POW) c.y = view(16384, one), c.y.p = nullptr;
    return c;
}

static void limits() {
    const size_t batch[1] = {3};
    const unsigned N[3] = {2, 3, 4}, one[3] = {1, 1, 1}, over[3] = {3, 683, 1}, over2[3] = {2, 2, 513}, at[3] = {2, 2, 512}, f64over[3] = {17, 241, 1};
    for (int op = 0; op < 6; ++op) {
        const std::string f(NAMES[op]);
        gft::SeriesArgs a;
        CHECK(verdict(call(op, N, N, batch, 1), &a).empty() && a.pl.w == 2 && a.g.items == 3);
        expect(call(op, N, over, batch, 1), f + ": n0 * n1 * n2 = 3 * 683 * 1 exceeds the limit of 2048 coefficients per item of this version");
        expect(call(op, N, over2, batch, 1), f + ": n0 * n1 * n2 = 2 * 2 * 513 exceeds the limit of 2048 coefficients per item of this version");
        CHECK(verdict(call(op, one, at, batch, 1)).empty());
        CHECK(verdict(call(op, one, over, batch, 1, 1)).empty());  // f64 keeps 4096
        expect(call(op, N, f64over, batch, 1, 1), f.substr(9) + ": n0 * n1 * n2 = 17 * 241 * 1 exceeds the limit of 4096 coefficients per item of this version");
    }
    CHECK(gft::series_limit(3, 1) == 4096 && gft::series_limit(3, 2) == 2048 && gft::SERIES3_MAX_ELEMS_IV == 2048);
    // an operation rank 3 lacks keeps its text byte for byte, for both widths
    for (int w = 1; w <= 2; ++w)
        for (int op : {gft::SERIES_CORR, gft::SERIES_COMPOSE_ADJ, gft::SERIES_DERIVATIVE, gft::SERIES_EVAL_ONE}) {
            gft::SeriesCall t = call(gft::SERIES_MUL, N, N, batch, 1, w);
            t.op = op, t.fn = "series3_other";
            expect(t, "series3_other: no such operation at rank 3 in this version (mul / div / exp / log on f64)");
        }
    gft::SeriesCall t = call(gft::SERIES_MUL, N, N, batch, 1);
    t.w = 3;
    expect(t, "interval series3_mul: no such operation at rank 3 in this version (mul / div / exp / log on f64)");
}

static void planes() {
    const size_t batch[2] = {3, 2};
    const unsigned N[3] = {2, 3, 4};  // 24 coefficients per item
    gft::SeriesArgs a;
    // null stride arrays: contiguous items, the planes back to back -- 6 items of 24
    CHECK(verdict(call(gft::SERIES_MUL, N, N, batch, 2), &a).empty());
    CHECK(a.pl.x == 144 && a.pl.y == 144 && a.pl.r == 144 && a.pl.s == 0 && a.g.nd == 1 && a.g.ext[0] == 6 && a.g.xs[0] == 24);
    // the plane stride is entry 0 of the array, the batch strides follow: planes interleaved per item (item stride 48, planes 24 apart)
    const int64_t inter[3] = {24, 96, 48}, point[3] = {0, 48, 24}, seeds[3] = {6, 2, 1};
    gft::SeriesCall c = call(gft::SERIES_MUL, N, N, batch, 2);
    c.x.bs = inter, c.y.bs = point, c.r.bs = inter;
    CHECK(verdict(c, &a).empty());
    CHECK(a.pl.x == 24 && a.pl.y == 0 && a.pl.r == 24 && a.g.nd == 1 && a.g.xs[0] == 48 && a.g.ys[0] == 24 && a.g.rs[0] == 48);
    // seeds [2, B...]: their plane stride too
    c = call(gft::SERIES_EXP, N, N, batch, 2);
    c.y.p = buffer + 16384, c.y.bs = seeds;
    CHECK(verdict(c, &a).empty() && a.pl.s == 6 && a.pl.y == 0 && a.g.ss[0] == 1);
    c.y.bs = point;  // point seeds
    CHECK(verdict(c, &a).empty() && a.pl.s == 0);
    const int64_t neg[3] = {-24, 96, 48};
    c = call(gft::SERIES_MUL, N, N, batch, 2);
    c.x.bs = neg;
    expect(c, "interval series3_mul: negative strides are not supported (x, the plane axis)");
    // the result's planes are distinct memory and join the distinct-address proof
    c = call(gft::SERIES_MUL, N, N, batch, 2);
    c.r.bs = point;
    expect(c, "interval series3_mul: the result has a zero plane stride: its lower and upper bounds overlap");
    const int64_t close[3] = {12, 48, 24};  // the upper bounds start inside the lower bounds of the same item (one slab in)
    c.r.bs = close;
    expect(c, "interval series3_mul: the result's series overlap each other (its strides do not separate the rows)");
    const int64_t slabwise[3] = {12, 96, 48};  // planes interleaved per SLAB: slab stride 24, planes 12 apart, items 48 apart
    c.r.bs = slabwise, c.r.st[0] = 24;
    CHECK(verdict(c, &a).empty() && a.pl.r == 12 && a.it.rs[0] == 24);
    // the overlap proof spans both planes: a result that starts inside x's upper plane
    c = call(gft::SERIES_MUL, N, N, batch, 2);
    c.r.p = buffer + 144 + 24;
    expect(c, "interval series3_mul: the result partially overlaps x (it may alias an operand only as the same view)");
    // the same memory with another plane stride is not the same view; the same view is in place
    c = call(gft::SERIES_POW, N, N, batch, 2);
    c.x.bs = point, c.r = view(0, N);
    expect(c, "interval series3_pow: the result partially overlaps x (it may alias an operand only as the same view)");
    c = call(gft::SERIES_POW, N, N, batch, 2);
    c.x.bs = inter, c.r = c.x;
    CHECK(verdict(c, &a).empty() && a.g.inplace == 1 && a.pl.x == 24 && a.pl.r == 24);
    c = call(gft::SERIES_COMPOSE, N, N, batch, 2);
    c.var = 2, c.y.bs = inter, c.r = c.y;
    CHECK(verdict(c, &a).empty() && a.g.inplace == 1);
    c.var = 3;
    expect(c, "interval series3_compose: var = 3 (the variable of f that g replaces is 0, 1 or 2)");
}

static void pow_cap() {
    // batch axes of 2, none contiguous with its neighbour on x (its strides alternate between 24 and 0; the result is contiguous).  The
    // copy carries the plane axis beside the batch axes, the slabs, the rows and the series: 9 where f64 takes 10
    const unsigned N[3] = {2, 3, 4};
    size_t b[11];
    int64_t xbs[12], rbs[12];
    int64_t rs = 24;
    for (int i = 10; i >= 0; --i) b[i] = 2, xbs[1 + i] = i % 2 ? 0 : 24, rbs[1 + i] = rs, rs *= 2;
    xbs[0] = 0, rbs[0] = rs;  // point intervals in, planes back to back out: 2 * 2^10 * 24 doubles
    gft::SeriesArgs a;
    gft::SeriesCall q = call(gft::SERIES_POW, N, N, b + 1, 10);
    int64_t x10[11], r10[11];
    x10[0] = 0, r10[0] = rs / 2;
    for (int i = 0; i < 10; ++i) x10[1 + i] = xbs[2 + i], r10[1 + i] = rbs[2 + i];
    q.x.bs = x10, q.r.bs = r10, q.r.p = buffer;
    q.x.p = buffer + 60000;
    expect(q, "interval series3_pow: the batch has more than 9 non-contiguous axes");
    q.w = 1, q.fn = "series3_pow", q.x.bs = x10 + 1, q.r.bs = r10 + 1;
    CHECK(verdict(q, &a).empty() && a.g.nd == 10);
    gft::SeriesCall p9 = call(gft::SERIES_POW, N, N, b + 2, 9);
    int64_t x9[10], r9[10];
    x9[0] = 0, r9[0] = rs / 4;
    for (int i = 0; i < 9; ++i) x9[1 + i] = xbs[3 + i], r9[1 + i] = rbs[3 + i];
    p9.x.bs = x9, p9.r.bs = r9, p9.r.p = buffer, p9.x.p = buffer + 60000;
    CHECK(verdict(p9, &a).empty() && a.g.nd == 9 && a.pl.x == 0 && a.pl.r == (size_t)(rs / 4));
    // the other operations carry one axis more (no slab and row axes in a copy of theirs)
    gft::SeriesCall m = call(gft::SERIES_MUL, N, N, b, 11);
    m.x.bs = xbs, m.y.bs = xbs, m.r.bs = rbs, m.r.p = buffer, m.x.p = m.y.p = buffer + 120000;
    CHECK(sizeof(buffer) / sizeof(double) >= (size_t)(2 * rs) && verdict(m, &a).empty() && a.g.nd == 11);
}

static gft::Series3Dims dims_of(int op, const unsigned* nx, const unsigned* ny, const unsigned* n) {
    const size_t xs[3] = {(size_t)nx[1] * nx[2], nx[2], 1}, ys[3] = {(size_t)ny[1] * ny[2], ny[2], 1}, rs[3] = {(size_t)n[1] * n[2], n[2], 1};
    return gft::series3_dims(op, nx, ny, n, xs, ys, rs);
}

static void sizes() {
    const size_t K80 = 80 * 1024, K64 = 64 * 1024;
    // (8, 8, 16): 1024 coefficients, two resident arrays of 16 KB each; pass 1 is chunked -- 7 * 8 terms of 128 elements against the
    // 3072 elements left of 80 KB
    const unsigned a[3] = {8, 8, 16};
    for (int op : {gft::SERIES_DIV, gft::SERIES_EXP, gft::SERIES_LOG}) {
        const gft::Series3Sizes z = gft::series3_sizes(op, dims_of(op, a, a, a), 2, K80);
        CHECK(z.fits && z.resident == 2048 && z.need == 128 && z.want == 56 * 128 && z.selems == 3072 && z.tc == 24);
        const gft::Series3Sizes f = gft::series3_sizes(op, dims_of(op, a, a, a), 1, K80);  // f64: every term at once
        CHECK(f.fits && f.selems == 56 * 128 && f.tc == 56);
    }
    // the limit: 64 KB resident, 1024 elements (16 KB) of scratch left -- eight slabs of 128 at (16, 16, 8), tc = 8; the one slab of
    // 1024 at (2, 2, 512), tc = 1
    const unsigned b[3] = {16, 16, 8}, c[3] = {2, 2, 512};
    gft::Series3Sizes z = gft::series3_sizes(gft::SERIES_DIV, dims_of(gft::SERIES_DIV, b, b, b), 2, K80);
    CHECK(z.fits && z.resident == 4096 && z.selems == 1024 && z.tc == 8);
    z = gft::series3_sizes(gft::SERIES_LOG, dims_of(gft::SERIES_LOG, c, c, c), 2, K80);
    CHECK(z.fits && z.resident == 4096 && z.need == 1024 && z.selems == 1024 && z.tc == 1);
    // under a 64 KB grant these do not fit; a compact divisor does
    CHECK(!gft::series3_sizes(gft::SERIES_DIV, dims_of(gft::SERIES_DIV, b, b, b), 2, K64).fits);
    CHECK(!gft::series3_sizes(gft::SERIES_LOG, dims_of(gft::SERIES_LOG, c, c, c), 2, K64).fits);
    const unsigned small[3] = {2, 2, 8};
    z = gft::series3_sizes(gft::SERIES_DIV, dims_of(gft::SERIES_DIV, b, small, b), 2, K64);
    CHECK(z.fits && z.resident == 2048 + 32 && z.tc == 2 && z.selems == 2 * 128);
    // the limit through the squeezes: one slab, the rank-2 sizes -- rows of n2 elements; one row (the rank-1 item): no scratch
    const unsigned r2[3] = {2, 1024, 1}, r1[3] = {1, 2048, 1};
    gft::Series3Dims d = dims_of(gft::SERIES_DIV, r2, r2, r2);
    CHECK(d.n[0] == 1 && d.n[1] == 2 && d.n[2] == 1024 && d.rs[1] == 1024 && d.rs[2] == 1);
    z = gft::series3_sizes(gft::SERIES_DIV, d, 2, K80);
    CHECK(z.fits && z.resident == 4096 && z.need == 1024 && z.selems == 1024 && z.tc == 0);
    d = dims_of(gft::SERIES_EXP, r1, r1, r1);
    CHECK(d.n[0] == 1 && d.n[1] == 1 && d.n[2] == 2048);
    z = gft::series3_sizes(gft::SERIES_EXP, d, 2, K64);
    CHECK(z.fits && z.need == 0 && z.selems == 0 && z.tc == 0);
    // the scratch never reaches past the budget
    for (unsigned n0 = 1; n0 <= 16; ++n0)
        for (unsigned n1 = 1; n1 <= 16; ++n1)
            for (unsigned n2 : {1u, 2u, 7u, 8u}) {
                const unsigned n[3] = {n0, n1, n2};
                for (int w = 1; w <= 2; ++w) {
                    const gft::Series3Sizes q = gft::series3_sizes(gft::SERIES_DIV, dims_of(gft::SERIES_DIV, n, n, n), w, K80);
                    CHECK(q.fits && (q.resident + q.selems) * 8 * w <= K80 && (q.need == 0 || q.selems >= q.need));
                }
            }
}

int main() {
    limits();
    planes();
    pow_cap();
    sizes();
    if (failures) {
        std::printf("FAILED %ld of %ld checks\n", failures, checks);
        return 1;
    }
    std::printf("ok %ld checks\n", checks);
    return 0;
}
