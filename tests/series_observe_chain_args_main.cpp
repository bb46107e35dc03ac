// The fused observation chain (SERIES_OBSERVE_CHAIN) in the host-side argument layer (genfer_amd/csrc/gft_series_args.hpp) on its own:
// no HIP, no device.  A self-checking program (tests/test_series_observe_chain_cpu.py builds and runs it, under the address and
// undefined-behaviour sanitizers where they are available; exit status 0 and a last line "ok <n> checks" when all holds):
//   * the shape rules with their texts and their order: the limit, var, nsteps, degree_p1, degree_p1 + nsteps <= L, the result;
//   * x and cs travel as the strides ys and ss of the batch with their plane strides, a null x is the continuous form;
//   * the result may overlap none of a, x and cs, and is never "the same view";
//   * rank 3 keeps its refusal.
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

// a chain on items (n0, n1) (rank 1: n0 == 1) along `var`: a at 0, x at 20000, cs at 24000, the result at 32768, its shape as the
// rules give it
static gft::SeriesCall chain(int rank, size_t n0, size_t n1, int var, size_t nsteps, size_t d, const size_t* batch, size_t nbatch, int w = 1) {
    gft::SeriesCall c;
    c.op = gft::SERIES_OBSERVE_CHAIN, c.w = w, c.rank = rank, c.var = rank == 1 ? 1 : var, c.batch = batch, c.nbatch = nbatch;
    c.fn = rank == 1 ? (w == 2 ? "interval series_observe_chain" : "series_observe_chain") : (w == 2 ? "interval series2_observe_chain" : "series2_observe_chain");
    c.nsteps = nsteps, c.degree_p1 = d;
    c.x = view(0, n0, n1), c.y = view(20000, 1, 1), c.cs = view(24000, 1, nsteps);
    const bool rows = rank == 2 && var == 0;
    const size_t o = std::min(rows ? n1 : n0, d);
    c.r = rank == 1 ? view(32768, 1, d) : (rows ? view(32768, d, o) : view(32768, o, d));
    return c;
}

static void rules() {
    const size_t batch[1] = {3};
    gft::SeriesArgs a;
    CHECK(verdict(chain(1, 1, 9, 1, 2, 7, batch, 1), &a).empty() && a.it.nx[2] == 9 && a.it.n[2] == 7 && a.g.items == 3);
    CHECK(verdict(chain(1, 1, 9, 1, 7, 2, batch, 1)).empty());
    expect(chain(1, 1, 9, 1, 0, 2, batch, 1), "series_observe_chain: nsteps = 0 (cs holds no constants: a chain has at least one step)");
    expect(chain(1, 1, 9, 1, 2, 1, batch, 1), "series_observe_chain: degree_p1 = 1 (the result needs at least two coefficients: degree_p1 >= 2)");
    expect(chain(1, 1, 9, 1, 2, 0, batch, 1), "series_observe_chain: degree_p1 = 0 (the result needs at least two coefficients: degree_p1 >= 2)");
    expect(chain(1, 1, 9, 1, 2, 8, batch, 1),
           "series_observe_chain: degree_p1 + nsteps = 8 + 2, but a has 9 stored coefficients (every step takes one: degree_p1 + nsteps <= 9)");
    expect(chain(1, 1, 9, 1, (size_t)-1, 8, batch, 1),
           "series_observe_chain: degree_p1 + nsteps = 8 + 18446744073709551615, but a has 9 stored coefficients (every step takes one: degree_p1 + nsteps <= 9)");
    expect(chain(1, 1, 9, 1, 2, 10, batch, 1),
           "series_observe_chain: degree_p1 + nsteps = 10 + 2, but a has 9 stored coefficients (every step takes one: degree_p1 + nsteps <= 9)");
    gft::SeriesCall c = chain(1, 1, 9, 1, 2, 7, batch, 1);
    c.r.len[2] = 6;
    expect(c, "series_observe_chain: the result has 6 coefficients; with degree_p1 = 7 it has 7");
    c = chain(1, 1, 0, 1, 2, 7, batch, 1);
    expect(c, "series_observe_chain: a has no coefficients");
    // the limits bound the operand: 4096 and 2048 pass, one more does not, and the limit is judged before the chain's own rules
    CHECK(verdict(chain(1, 1, 4096, 1, 64, 4032, batch, 1)).empty());
    expect(chain(1, 1, 4097, 1, 0, 0, batch, 1), "series_observe_chain: na = 4097 exceeds the limit of 4096 coefficients per series of this version");
    CHECK(verdict(chain(1, 1, 2048, 1, 64, 1984, batch, 1, 2)).empty());
    expect(chain(1, 1, 2049, 1, 1, 2, batch, 1, 2), "interval series_observe_chain: na = 2049 exceeds the limit of 2048 coefficients per series of this version");
    // rank 2: the axis, the lengths on it, the result's other axis cut to min(len, degree_p1)
    CHECK(verdict(chain(2, 5, 7, 1, 2, 3, batch, 1), &a).empty() && a.it.n[1] == 3 && a.it.n[2] == 3 && a.it.xs[1] == 7);
    CHECK(verdict(chain(2, 5, 7, 0, 2, 3, batch, 1), &a).empty() && a.it.n[1] == 3 && a.it.n[2] == 3);
    CHECK(verdict(chain(2, 1, 9, 1, 2, 3, batch, 1), &a).empty() && a.it.n[1] == 1 && a.it.n[2] == 3);
    CHECK(verdict(chain(2, 9, 1, 0, 7, 2, batch, 1), &a).empty() && a.it.n[1] == 2 && a.it.n[2] == 1);
    CHECK(verdict(chain(2, 64, 64, 0, 16, 48, batch, 1)).empty());
    for (int var : {2, -1})
        expect(chain(2, 5, 7, var, 2, 3, batch, 1), "series2_observe_chain: var = " + std::to_string(var) + " (the variable the operation acts on is 0 or 1)");
    expect(chain(2, 5, 7, 0, 2, 4, batch, 1),
           "series2_observe_chain: degree_p1 + nsteps = 4 + 2, but a has 5 stored coefficients on axis 0 (every step takes one: degree_p1 + nsteps <= 5)");
    expect(chain(2, 5, 7, 1, 2, 1, batch, 1), "series2_observe_chain: degree_p1 = 1 (the result needs at least two coefficients on axis 1: degree_p1 >= 2)");
    c = chain(2, 5, 7, 1, 2, 3, batch, 1);
    c.r.len[1] = 5;
    expect(c, "series2_observe_chain: the result has 5 x 3 coefficients; with degree_p1 = 3 it has 3 x 3");
    expect(chain(2, 64, 65, 1, 2, 3, batch, 1), "series2_observe_chain: a has 64 * 65 coefficients, which exceeds the limit of 4096 coefficients per item of this version");
    expect(chain(2, 32, 65, 1, 2, 3, batch, 1, 2),
           "interval series2_observe_chain: a has 32 * 65 coefficients, which exceeds the limit of 2048 coefficients per item of this version");
    // rank 3 has no such operation: the pinned text
    c = chain(2, 5, 7, 1, 2, 3, batch, 1);
    c.rank = 3, c.fn = "series3_observe_chain";
    expect(c, "series3_observe_chain: no such operation at rank 3 in this version (mul / div / exp / log on f64)");
    // an empty batch: nothing to do, no stride looked at
    const size_t none[2] = {3, 0};
    bool ran = true;
    CHECK(verdict(chain(1, 1, 9, 1, 2, 7, none, 2), nullptr, &ran).empty() && !ran);
}

static void scalars() {
    const size_t batch[2] = {3, 2};
    gft::SeriesArgs a;
    // null stride arrays: contiguous items; x one per item, cs nsteps per item
    CHECK(verdict(chain(1, 1, 9, 1, 2, 7, batch, 2), &a).empty());
    CHECK(a.g.nd == 1 && a.g.ext[0] == 6 && a.g.xs[0] == 9 && a.g.ys[0] == 1 && a.g.ss[0] == 2 && a.g.rs[0] == 7);
    // stride 0 on x and on cs: one scalar for every item, one set of constants per column of the batch
    const int64_t x0[2] = {0, 0}, c0[2] = {0, 2};
    gft::SeriesCall c = chain(1, 1, 9, 1, 2, 7, batch, 2);
    c.y.bs = x0, c.cs.bs = c0;
    CHECK(verdict(c, &a).empty() && a.g.nd == 2 && a.g.ys[0] == 0 && a.g.ys[1] == 0 && a.g.ss[0] == 0 && a.g.ss[1] == 2);
    // the continuous form: no x, its strides stay 0
    c = chain(1, 1, 9, 1, 2, 7, batch, 2);
    c.y.p = nullptr;
    CHECK(verdict(c, &a).empty() && a.g.nd == 1 && a.g.ys[0] == 0 && a.pl.y == 0 && a.g.ss[0] == 2);
    // intervals: the plane stride leads every array; null arrays are planes back to back
    CHECK(verdict(chain(1, 1, 9, 1, 2, 7, batch, 2, 2), &a).empty());
    CHECK(a.pl.x == 54 && a.pl.y == 6 && a.pl.s == 12 && a.pl.r == 42);
    const int64_t xp[3] = {0, 2, 1}, cp[3] = {0, 4, 2};  // point scalars
    c = chain(1, 1, 9, 1, 2, 7, batch, 2, 2);
    c.y.bs = xp, c.cs.bs = cp;
    CHECK(verdict(c, &a).empty() && a.pl.y == 0 && a.pl.s == 0 && a.g.ys[0] == 1 && a.g.ss[0] == 2);
    const int64_t neg[2] = {-2, 1};
    c = chain(1, 1, 9, 1, 2, 7, batch, 2);
    c.cs.bs = neg;
    expect(c, "series_observe_chain: negative strides are not supported (cs, batch axis 0)");
    c = chain(1, 1, 9, 1, 2, 7, batch, 2);
    c.y.bs = neg;
    expect(c, "series_observe_chain: negative strides are not supported (x, batch axis 0)");
}

static void overlaps() {
    const size_t batch[1] = {3};
    // the result inside a, on x, on cs: each refused by address range; a result that starts at a is no "same view"
    gft::SeriesCall c = chain(1, 1, 9, 1, 2, 7, batch, 1);
    c.r.p = buffer + 1;
    expect(c, "series_observe_chain: the result partially overlaps a (it may alias an operand only as the same view)");
    c.r.p = buffer;
    expect(c, "series_observe_chain: the result partially overlaps a (it may alias an operand only as the same view)");
    c = chain(1, 1, 9, 1, 2, 7, batch, 1);
    c.y.p = buffer + 32768 + 20;
    expect(c, "series_observe_chain: the result partially overlaps x (it may alias an operand only as the same view)");
    c = chain(1, 1, 9, 1, 2, 7, batch, 1);
    c.cs.p = buffer + 32768 + 18;
    expect(c, "series_observe_chain: the result partially overlaps cs (it may alias an operand only as the same view)");
    c.cs.p = buffer + 32768 + 21;  // just behind the result's last element
    CHECK(verdict(c).empty());
    const int64_t zero[1] = {0};
    c = chain(1, 1, 9, 1, 2, 7, batch, 1);
    c.r.bs = zero;
    expect(c, "series_observe_chain: the result has a zero stride (batch axis 0): its series overlap");
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
