// BigFloat calls (elem == SERIES_ELEM_BIGFLOAT, w == 2) in the host-side argument layer (genfer_amd/csrc/gft_series_args.hpp) on their
// own: no HIP, no device.  A self-checking program (tests/test_bigfloat_series_cpu.py builds and runs it, under the address and
// undefined-behaviour sanitizers where they are available; exit status 0 and a last line "ok <n> checks" when all holds):
//   * the six arithmetic operations are admitted at rank 1 with the interval limit of 2048 and its text;
//   * every other rank and every other operation is refused, by the function's name;
//   * a plane stride of 0 is refused on an operand, on the seeds and (as for intervals) on the result;
//   * everything else is the interval path's judgement: the plane stride leads the stride arrays, a null array means planes back to
//     back, overlap, the result as an operand's same view, the batch collapse;
//   * the default element kind leaves an interval call and an f64 call exactly as they were (the same calls with `elem` untouched).
#include <cstdio>
#include <string>

#include "../genfer_amd/csrc/gft_series_args.hpp"

static double buffer[1 << 16];
static long checks = 0, failures = 0;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++checks;                                                                     \
        if (!(cond)) {                                                                \
            if (++failures <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                             \
    } while (0)

static gft::SeriesView view(size_t off, size_t len, const int64_t* bs = nullptr) {
    gft::SeriesView v;
    v.p = buffer + off, v.bs = bs;
    v.len[2] = len;
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

static const char* NAMES[6] = {"bigfloat series_mul", "bigfloat series_div", "bigfloat series_exp", "bigfloat series_log",
                               "bigfloat series_compose", "bigfloat series_pow"};

// a call of operation `op` on rows of nx and n, x at 0, y at 16384, the result at 32768 (planes back to back unless bs says otherwise);
// exp / log without seeds
static gft::SeriesCall call(int op, size_t nx, size_t n, const size_t* batch, size_t nbatch, int elem = gft::SERIES_ELEM_BIGFLOAT, int w = 2) {
    gft::SeriesCall c;
    c.op = op, c.fn = op < 6 ? NAMES[op] : "bigfloat series_other", c.w = w, c.elem = elem, c.rank = 1, c.batch = batch, c.nbatch = nbatch, c.e = 5;
    c.x = view(0, nx), c.r = view(32768, n);
    if (op == gft::SERIES_MUL || op == gft::SERIES_DIV || op == gft::SERIES_COMPOSE) c.y = view(16384, nx);
    else if (op != gft::SERIES_POW) c.y = view(16384, 1), c.y.p = nullptr;
    return c;
}

static void admitted() {
    const size_t batch[2] = {3, 2};
    for (int op = 0; op < 6; ++op) {
        const std::string f(NAMES[op]);
        gft::SeriesArgs a;
        CHECK(verdict(call(op, 5, 9, batch, 2), &a).empty());
        CHECK(a.pl.w == 2 && a.pl.elem == gft::SERIES_ELEM_BIGFLOAT && a.g.items == 6 && a.g.nd == 1 && a.g.ext[0] == 6);
        CHECK(a.pl.x == 30 && a.pl.r == 54 && a.it.nx[2] == 5 && a.it.n[2] == 9);  // null stride arrays: the planes back to back
        CHECK(verdict(call(op, 5, 2048, batch, 1)).empty());
        expect(call(op, 5, 2049, batch, 1), f + ": n = 2049 exceeds the limit of 2048 coefficients per series of this version");
        expect(call(op, 5, 0, batch, 1), f + ": n == 0 (the result has no coefficients)");
        expect(call(op, 9, 5, batch, 1), f + ": nx = 9 > n = 5 (an operand is longer than the truncation order)");
    }
    const size_t none[1] = {0};
    gft::SeriesArgs a;
    gft::SeriesCall c = call(gft::SERIES_MUL, 5, 9, none, 1);
    bool ran = true;
    try {
        ran = gft::series_args(c, a, [](const double*, const char*) {});
    } catch (const std::exception&) {
    }
    CHECK(!ran);  // an empty batch: nothing to do, as for every family
}

static void other_ranks_and_ops() {
    const size_t batch[1] = {3};
    for (int rank = 2; rank <= 3; ++rank)
        for (int op = 0; op < 6; ++op) {
            gft::SeriesCall c = call(op, 4, 4, batch, 1);
            c.rank = rank;
            expect(c, std::string(NAMES[op]) + ": BigFloat series exist at rank 1 only in this version (rank " + std::to_string(rank) + " was asked for)");
        }
    for (int op = gft::SERIES_CORR; op < gft::SERIES_OP_COUNT; ++op) {
        gft::SeriesCall c = call(op, 4, 4, batch, 1);
        c.y = view(16384, 4), c.cs = view(20000, 1), c.nsteps = 1, c.degree_p1 = 2, c.var = 1, c.wvar = 1;
        expect(c, "bigfloat series_other: no such operation on BigFloat series in this version (mul / div / exp / log / compose / pow)");
    }
    gft::SeriesCall c = call(gft::SERIES_MUL, 4, 4, batch, 1);
    c.w = 1;
    expect(c, "bigfloat series_mul: a BigFloat tensor has two planes (factor, exponent), not 1");
}

static void planes() {
    const size_t batch[2] = {3, 2};
    const int64_t inter[3] = {8, 32, 16}, point[3] = {0, 16, 8}, seeds[3] = {6, 2, 1}, pseeds[3] = {0, 2, 1};
    gft::SeriesArgs a;
    // the plane stride is entry 0 of the array, the batch strides follow: planes interleaved per item (item stride 16, planes 8 apart)
    gft::SeriesCall c = call(gft::SERIES_MUL, 8, 8, batch, 2);
    c.x.bs = inter, c.y.bs = inter, c.r.bs = inter;
    CHECK(verdict(c, &a).empty() && a.pl.x == 8 && a.pl.y == 8 && a.pl.r == 8 && a.g.nd == 1 && a.g.xs[0] == 16 && a.g.rs[0] == 16);
    // a zero plane stride: refused on either operand, on the seeds, on the result
    c.x.bs = point;
    expect(c, "bigfloat series_mul: zero plane stride on x (the factor plane of a BigFloat tensor cannot be its own exponent plane)");
    c.x.bs = inter, c.y.bs = point;
    expect(c, "bigfloat series_mul: zero plane stride on y (the factor plane of a BigFloat tensor cannot be its own exponent plane)");
    c = call(gft::SERIES_COMPOSE, 8, 8, batch, 2);
    c.y.bs = point;
    expect(c, "bigfloat series_compose: zero plane stride on g (the factor plane of a BigFloat tensor cannot be its own exponent plane)");
    c.y.bs = nullptr, c.x.bs = point;
    expect(c, "bigfloat series_compose: zero plane stride on f (the factor plane of a BigFloat tensor cannot be its own exponent plane)");
    c = call(gft::SERIES_POW, 8, 8, batch, 2);
    c.x.bs = point;
    expect(c, "bigfloat series_pow: zero plane stride on x (the factor plane of a BigFloat tensor cannot be its own exponent plane)");
    for (int op : {gft::SERIES_EXP, gft::SERIES_LOG}) {
        c = call(op, 8, 8, batch, 2);
        CHECK(verdict(c, &a).empty() && a.pl.s == 0);  // no seeds: nothing to judge about them
        c.y.p = buffer + 16384, c.y.bs = seeds;
        CHECK(verdict(c, &a).empty() && a.pl.s == 6 && a.g.ss[0] == 1);
        c.y.bs = pseeds;
        expect(c, std::string(NAMES[op]) + ": zero plane stride on the seeds (the factor plane of a BigFloat tensor cannot be its own exponent plane)");
    }
    c = call(gft::SERIES_MUL, 8, 8, batch, 2);
    c.r.bs = point;
    expect(c, "bigfloat series_mul: the result has a zero plane stride: its lower and upper bounds overlap");
    // the interval path's judgement unchanged: negative strides, the result's planes in the distinct-address proof, overlap, same view
    const int64_t neg[3] = {-8, 32, 16}, close[3] = {4, 32, 16};
    c = call(gft::SERIES_MUL, 8, 8, batch, 2);
    c.x.bs = neg;
    expect(c, "bigfloat series_mul: negative strides are not supported (x, the plane axis)");
    c.x.bs = nullptr, c.r.bs = close;
    expect(c, "bigfloat series_mul: the result's series overlap each other (its strides do not separate the rows)");
    c = call(gft::SERIES_MUL, 8, 8, batch, 2);
    c.r.p = buffer + 48 + 8;  // inside x's exponent plane
    expect(c, "bigfloat series_mul: the result partially overlaps x (it may alias an operand only as the same view)");
    c = call(gft::SERIES_MUL, 8, 8, batch, 2);
    c.x.bs = inter, c.r = c.x;
    CHECK(verdict(c, &a).empty() && a.g.inplace == 1 && a.pl.x == 8 && a.pl.r == 8);
    c = call(gft::SERIES_DIV, 8, 8, batch, 2);
    c.r = c.y;
    CHECK(verdict(c, &a).empty() && a.g.inplace == 1);
    c = call(gft::SERIES_POW, 8, 8, batch, 2);
    c.x.bs = inter, c.r = view(0, 8);  // the same memory with another plane stride is not the same view
    expect(c, "bigfloat series_pow: the result partially overlaps x (it may alias an operand only as the same view)");
    // one series against every item: a batch stride of 0 is a value on an operand
    const int64_t one[3] = {8, 0, 0};
    c = call(gft::SERIES_MUL, 8, 8, batch, 2);
    c.y.bs = one;
    CHECK(verdict(c, &a).empty() && a.g.nd == 1 && a.g.ys[0] == 0 && a.pl.y == 8);
}

// the default element kind: an interval call and an f64 call, written as every caller from before the element kind writes them
static void defaults_untouched() {
    const size_t batch[2] = {3, 2};
    const int64_t point[3] = {0, 16, 8};
    gft::SeriesArgs a;
    gft::SeriesCall c;
    CHECK(c.elem == gft::SERIES_ELEM_BY_WIDTH && gft::SeriesPlanes().elem == gft::SERIES_ELEM_BY_WIDTH);
    c.op = gft::SERIES_MUL, c.fn = "interval series_mul", c.w = 2, c.batch = batch, c.nbatch = 2;
    c.x = view(0, 8, point), c.y = view(16384, 8), c.r = view(32768, 8);
    CHECK(verdict(c, &a).empty());  // a point interval: the plane stride 0 stays a value
    CHECK(a.pl.w == 2 && a.pl.elem == gft::SERIES_ELEM_BY_WIDTH && a.pl.x == 0 && a.pl.y == 48 && a.pl.r == 48 && a.g.nd == 1 && a.g.items == 6 && a.g.xs[0] == 8);
    c.rank = 2, c.fn = "interval series2_mul";  // rank 2 is still there for intervals
    c.x = view(0, 8), c.x.len[1] = 2, c.x.st[1] = 8, c.y = view(16384, 8), c.y.len[1] = 2, c.y.st[1] = 8, c.r = view(32768, 8), c.r.len[1] = 2, c.r.st[1] = 8;
    CHECK(verdict(c, &a).empty() && a.pl.x == 96 && a.it.n[1] == 2);
    gft::SeriesCall d;
    d.op = gft::SERIES_CORR, d.fn = "series_corr", d.batch = batch, d.nbatch = 2;
    d.x = view(0, 8), d.y = view(16384, 4), d.r = view(32768, 8);
    CHECK(verdict(d, &a).empty() && a.pl.w == 1 && a.pl.elem == gft::SERIES_ELEM_BY_WIDTH && a.pl.x == 0 && a.g.items == 6 && a.g.xs[0] == 8 && a.g.ys[0] == 4);
    d.r = view(32768, 4097), d.op = gft::SERIES_MUL, d.fn = "series_mul";
    expect(d, "series_mul: n = 4097 exceeds the limit of 4096 coefficients per series of this version");
}

int main() {
    admitted();
    other_ranks_and_ops();
    planes();
    defaults_untouched();
    if (failures) {
        std::printf("FAILED %ld of %ld checks\n", failures, checks);
        return 1;
    }
    std::printf("ok %ld checks\n", checks);
    return 0;
}
