// The affine substitutions (SERIES_MUL_LINEAR, SERIES_COMPOSE_LINEAR) in the host-side argument layer
// (genfer_amd/csrc/gft_series_args.hpp) on its own: no HIP, no device.  A self-checking program (tests/test_series_linear_cpu.py builds
// and runs it, under the address and undefined-behaviour sanitizers where they are available; exit status 0 and a last line
// "ok <n> checks" when all holds):
//   * the shape rules with their texts: var and wvar, two coefficients on the affine series' axis, the operand inside the result, the
//     limit on the result;
//   * c and m travel as the strides ys and ss of the batch with their plane strides;
//   * the result may overlap none of the operand, c and m, and is never "the same view";
//   * rank 3 keeps its pinned refusal for both operations and both widths; an empty batch is a no-op.
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

static std::string verdict(const gft::SeriesCall& c, gft::SeriesArgs* out = nullptr, bool* ran = nullptr) {
    try {
        gft::SeriesArgs a;
        const bool r = gft::series_args(c, a, [](const double*, const char*) {});
        if (out) *out = a;
        if (ran) *ran = r;
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

static gft::SeriesView view(size_t off, size_t len1, size_t len2, const int64_t* bs = nullptr) {
    gft::SeriesView v;
    v.p = buffer + off, v.bs = bs;
    v.len[1] = len1, v.len[2] = len2;
    v.st[1] = (int64_t)len2;
    return v;
}

// a call on items (a0, a1) (rank 1: a0 == 1) at the orders (n0, n1): the operand at 0, c at 20000, m at 24000, the result at 32768
static gft::SeriesCall call(int op, int rank, size_t a0, size_t a1, int var, int wvar, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                            int w = 1) {
    static std::string names[16];
    gft::SeriesCall c;
    c.op = op, c.w = w, c.rank = rank, c.batch = batch, c.nbatch = nbatch;
    c.var = rank == 1 ? 1 : var, c.wvar = rank == 1 ? 1 : wvar;
    std::string& fn = names[(op == gft::SERIES_MUL_LINEAR) + 2 * (rank - 1) + 6 * (w == 2)];
    fn = std::string(w == 2 ? "interval " : "") + (rank == 1 ? "series_" : (rank == 2 ? "series2_" : "series3_")) +
         (op == gft::SERIES_MUL_LINEAR ? "mul_linear" : "compose_linear");
    c.fn = fn.c_str();
    c.x = view(0, a0, a1), c.y = view(20000, 1, 1), c.cs = view(24000, 1, 1), c.r = view(32768, n0, n1);
    return c;
}
static const int MUL = gft::SERIES_MUL_LINEAR, COMP = gft::SERIES_COMPOSE_LINEAR;

static void rules() {
    const size_t batch[1] = {3};
    gft::SeriesArgs a;
    CHECK(verdict(call(COMP, 1, 1, 9, 1, 1, 1, 12, batch, 1), &a).empty() && a.it.nx[2] == 9 && a.it.n[2] == 12 && a.g.items == 3);
    CHECK(verdict(call(MUL, 1, 1, 9, 1, 1, 1, 10, batch, 1), &a).empty() && a.it.nx[2] == 9 && a.it.n[2] == 10);
    CHECK(verdict(call(MUL, 1, 1, 9, 1, 1, 1, 9, batch, 1)).empty());
    CHECK(verdict(call(COMP, 1, 1, 1, 1, 1, 1, 2, batch, 1)).empty());
    // a substitution at one coefficient is not linear
    expect(call(COMP, 1, 1, 1, 1, 1, 1, 1, batch, 1),
           "series_compose_linear: the result has 1 coefficient (c + m * x needs two: a substitution at one coefficient is the constant one, not a linear one)");
    expect(call(MUL, 1, 1, 1, 1, 1, 1, 1, batch, 1),
           "series_mul_linear: the result has 1 coefficient (c + m * x needs two: a substitution at one coefficient is the constant one, not a linear one)");
    expect(call(COMP, 2, 5, 7, 0, 1, 5, 1, batch, 1),
           "series2_compose_linear: the result has 1 coefficient on axis -1 (c + m * x needs two: a substitution at one coefficient is the constant one, not a "
           "linear one)");
    expect(call(MUL, 2, 1, 7, 0, 0, 1, 7, batch, 1),
           "series2_mul_linear: the result has 1 coefficient on axis -2 (c + m * x needs two: a substitution at one coefficient is the constant one, not a linear "
           "one)");
    CHECK(verdict(call(COMP, 2, 1, 7, 1, 1, 1, 7, batch, 1)).empty());  // one coefficient on the OTHER axis is fine
    expect(call(COMP, 1, 1, 9, 1, 1, 1, 0, batch, 1), "series_compose_linear: n == 0 (the result has no coefficients)");
    expect(call(MUL, 2, 5, 7, 1, 1, 0, 8, batch, 1), "series2_mul_linear: n0 * n1 == 0 (the result has no coefficients)");
    expect(call(MUL, 1, 1, 0, 1, 1, 1, 4, batch, 1), "series_mul_linear: an operand has no coefficients");
    // the axes
    for (int var : {2, -1}) {
        expect(call(COMP, 2, 5, 7, var, 1, 5, 7, batch, 1),
               "series2_compose_linear: var = " + std::to_string(var) + " (the variable of f that is replaced is 0 or 1)");
        expect(call(MUL, 2, 5, 7, var, var, 5, 8, batch, 1),
               "series2_mul_linear: var = " + std::to_string(var) + " (the variable of the linear factor is 0 or 1)");
        expect(call(COMP, 2, 5, 7, 1, var, 5, 7, batch, 1),
               "series2_compose_linear: wvar = " + std::to_string(var) + " (the variable of the affine series is 0 or 1)");
    }
    // the operand lies inside the result
    expect(call(COMP, 1, 1, 9, 1, 1, 1, 8, batch, 1), "series_compose_linear: nf = 9 > n = 8 (an operand is longer than the truncation order)");
    expect(call(MUL, 1, 1, 9, 1, 1, 1, 8, batch, 1), "series_mul_linear: na = 9 > n = 8 (an operand is longer than the truncation order)");
    expect(call(COMP, 2, 5, 7, 0, 1, 4, 9, batch, 1),
           "series2_compose_linear: f has 5 x 7 coefficients, the result 4 x 9 (an operand is longer than the truncation order)");
    expect(call(MUL, 2, 5, 7, 0, 0, 6, 6, batch, 1),
           "series2_mul_linear: a has 5 x 7 coefficients, the result 6 x 6 (an operand is longer than the truncation order)");
    // the limits bound the result: 4096 and 2048 pass, one more does not
    CHECK(verdict(call(COMP, 1, 1, 4096, 1, 1, 1, 4096, batch, 1)).empty());
    CHECK(verdict(call(MUL, 1, 1, 4095, 1, 1, 1, 4096, batch, 1)).empty());
    expect(call(COMP, 1, 1, 9, 1, 1, 1, 4097, batch, 1), "series_compose_linear: n = 4097 exceeds the limit of 4096 coefficients per series of this version");
    CHECK(verdict(call(COMP, 1, 1, 2048, 1, 1, 1, 2048, batch, 1, 2)).empty());
    expect(call(MUL, 1, 1, 9, 1, 1, 1, 2049, batch, 1, 2),
           "interval series_mul_linear: n = 2049 exceeds the limit of 2048 coefficients per series of this version");
    CHECK(verdict(call(COMP, 2, 64, 64, 0, 1, 64, 64, batch, 1)).empty());
    expect(call(COMP, 2, 5, 7, 0, 1, 64, 65, batch, 1),
           "series2_compose_linear: n0 * n1 = 64 * 65 exceeds the limit of 4096 coefficients per item of this version");
    expect(call(MUL, 2, 5, 7, 1, 1, 32, 65, batch, 1, 2),
           "interval series2_mul_linear: n0 * n1 = 32 * 65 exceeds the limit of 2048 coefficients per item of this version");
    // rank 2: an accepted call's item
    CHECK(verdict(call(COMP, 2, 5, 7, 0, 1, 6, 11, batch, 1), &a).empty() && a.it.nx[1] == 5 && a.it.nx[2] == 7 && a.it.n[1] == 6 && a.it.n[2] == 11 &&
          a.it.xs[1] == 7 && a.it.rs[1] == 11);
    // rank 3 has no such operation: the pinned text, for both operations and both widths
    for (int op : {MUL, COMP})
        for (int w : {1, 2}) {
            gft::SeriesCall c = call(op, 3, 5, 7, 1, 1, 5, 8, batch, 1, w);
            expect(c, std::string(c.fn) + ": no such operation at rank 3 in this version (mul / div / exp / log on f64)");
        }
    // an empty batch: nothing to do, no stride looked at
    const size_t none[2] = {3, 0};
    for (int op : {MUL, COMP}) {
        bool ran = true;
        CHECK(verdict(call(op, 1, 1, 9, 1, 1, 1, 12, none, 2), nullptr, &ran).empty() && !ran);
    }
}

static void scalars() {
    const size_t batch[2] = {3, 2};
    gft::SeriesArgs a;
    // null stride arrays: contiguous items, one c and one m per item; the batch collapses to one axis
    CHECK(verdict(call(COMP, 1, 1, 9, 1, 1, 1, 12, batch, 2), &a).empty());
    CHECK(a.g.nd == 1 && a.g.ext[0] == 6 && a.g.xs[0] == 9 && a.g.ys[0] == 1 && a.g.ss[0] == 1 && a.g.rs[0] == 12 && !a.g.inplace);
    // stride 0 on c, m per column of the batch: the axes stay apart
    const int64_t c0[2] = {0, 0}, m0[2] = {0, 1};
    gft::SeriesCall c = call(MUL, 1, 1, 9, 1, 1, 1, 10, batch, 2);
    c.y.bs = c0, c.cs.bs = m0;
    CHECK(verdict(c, &a).empty() && a.g.nd == 2 && a.g.ys[0] == 0 && a.g.ys[1] == 0 && a.g.ss[0] == 0 && a.g.ss[1] == 1);
    // intervals: the plane stride leads every array; null arrays are planes back to back
    CHECK(verdict(call(COMP, 1, 1, 9, 1, 1, 1, 12, batch, 2, 2), &a).empty());
    CHECK(a.pl.x == 54 && a.pl.y == 6 && a.pl.s == 6 && a.pl.r == 72);
    const int64_t cp[3] = {0, 2, 1}, mp[3] = {0, 2, 1};  // point scalars
    c = call(COMP, 1, 1, 9, 1, 1, 1, 12, batch, 2, 2);
    c.y.bs = cp, c.cs.bs = mp;
    CHECK(verdict(c, &a).empty() && a.pl.y == 0 && a.pl.s == 0 && a.g.ys[0] == 1 && a.g.ss[0] == 1);
    const int64_t neg[2] = {-2, 1};
    c = call(COMP, 1, 1, 9, 1, 1, 1, 12, batch, 2);
    c.cs.bs = neg;
    expect(c, "series_compose_linear: negative strides are not supported (m, batch axis 0)");
    c = call(MUL, 1, 1, 9, 1, 1, 1, 10, batch, 2);
    c.y.bs = neg;
    expect(c, "series_mul_linear: negative strides are not supported (c, batch axis 0)");
    c = call(MUL, 1, 1, 9, 1, 1, 1, 10, batch, 2);
    c.x.bs = neg;
    expect(c, "series_mul_linear: negative strides are not supported (a, batch axis 0)");
}

static void overlaps() {
    const size_t batch[1] = {3};
    // the result inside the operand, on c, on m: each refused by address range; a result that IS the operand's view is refused too
    gft::SeriesCall c = call(COMP, 1, 1, 9, 1, 1, 1, 12, batch, 1);
    c.r.p = buffer + 1;
    expect(c, "series_compose_linear: the result partially overlaps f (it may alias an operand only as the same view)");
    c = call(COMP, 1, 1, 9, 1, 1, 1, 9, batch, 1);
    c.r.p = buffer;
    expect(c, "series_compose_linear: the result partially overlaps f (it may alias an operand only as the same view)");
    c = call(MUL, 1, 1, 9, 1, 1, 1, 9, batch, 1);
    c.r.p = buffer;
    expect(c, "series_mul_linear: the result partially overlaps a (it may alias an operand only as the same view)");
    c = call(MUL, 1, 1, 9, 1, 1, 1, 10, batch, 1);
    c.y.p = buffer + 32768 + 29;
    expect(c, "series_mul_linear: the result partially overlaps c (it may alias an operand only as the same view)");
    c = call(COMP, 1, 1, 9, 1, 1, 1, 12, batch, 1);
    c.cs.p = buffer + 32768 + 35;
    expect(c, "series_compose_linear: the result partially overlaps m (it may alias an operand only as the same view)");
    c.cs.p = buffer + 32768 + 36;  // just behind the result's last element
    CHECK(verdict(c).empty());
    const int64_t zero[1] = {0};
    c = call(COMP, 1, 1, 9, 1, 1, 1, 12, batch, 1);
    c.r.bs = zero;
    expect(c, "series_compose_linear: the result has a zero stride (batch axis 0): its series overlap");
}

int main() {
    rules();
    scalars();
    overlaps();
    if (failures) {
        std::printf("FAILED %ld of %ld checks\n", failures, checks);
        return 1;
    }
    std::printf("ok %ld checks\n", checks);
    return 0;
}
