// The negative-binomial observation (SERIES_OBSERVE_NEGBINOMIAL) and the Lah row (SERIES_LAH_ROW) in the host-side argument layer
// (genfer_amd/csrc/gft_series_args.hpp) on their own: no HIP, no device.  A self-checking program
// (tests/test_series_observe_negbinomial_cpu.py builds and runs it, also under the address and undefined-behaviour sanitizers; exit
// status 0 and a last line "ok <n> checks" when all holds):
//   * the shape rules with their whole texts and their order: the empty operand, the limit, var, then the row, degree_p1 >= 3,
//     degree_p1 + order <= L, the operation's own limit, the result;
//   * x, p and ls travel as the strides ys, SeriesArgs::ps and ss of the batch with their plane strides, and one accepted call's
//     collapsed batch;
//   * the result may overlap none of a, x, p and ls, judged by address range;
//   * rank 3 and BigFloat keep their refusals, in front of every new check.
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

// an observation on items (n0, n1) (rank 1: n0 == 1) along `var` with a row of nls entries: a at 0, x at 20000, p at 22000, ls at
// 24000, the result at 32768, its shape as the rules give it
static gft::SeriesCall negbin(int rank, size_t n0, size_t n1, int var, size_t nls, size_t d, const size_t* batch, size_t nbatch, int w = 1) {
    gft::SeriesCall c;
    c.op = gft::SERIES_OBSERVE_NEGBINOMIAL, c.w = w, c.rank = rank, c.var = rank == 1 ? 1 : var, c.batch = batch, c.nbatch = nbatch;
    c.fn = rank == 1 ? (w == 2 ? "interval series_observe_negbinomial" : "series_observe_negbinomial")
                     : (w == 2 ? "interval series2_observe_negbinomial" : "series2_observe_negbinomial");
    c.nsteps = nls, c.degree_p1 = d;
    c.x = view(0, n0, n1), c.y = view(20000, 1, 1), c.p = view(22000, 1, 1), c.cs = view(24000, 1, nls);
    const bool rows = rank == 2 && var == 0;
    const size_t o = std::min(rows ? n1 : n0, d);
    c.r = rank == 1 ? view(32768, 1, d) : (rows ? view(32768, d, o) : view(32768, o, d));
    return c;
}

static gft::SeriesCall lah(size_t order, const size_t* batch, size_t nbatch, int w = 1) {
    gft::SeriesCall c;
    c.op = gft::SERIES_LAH_ROW, c.w = w, c.rank = 1, c.var = 1, c.batch = batch, c.nbatch = nbatch;
    c.fn = w == 2 ? "interval series_lah_row" : "series_lah_row";
    c.x = view(0, 1, 1), c.r = view(32768, 1, order + 1);
    return c;
}

static void rules() {
    const size_t batch[1] = {3};
    gft::SeriesArgs a;
    // the two rows lie behind the table: SERIES_OPS keeps its fifteen rows, series_op_row finds either kind
    CHECK(gft::SERIES_OP_COUNT == 15 && sizeof(gft::SERIES_OPS) / sizeof(gft::SERIES_OPS[0]) == 15);
    CHECK(std::string(gft::series_op_row(gft::SERIES_OBSERVE_NEGBINOMIAL).cs) == "ls" && gft::series_op_row(gft::SERIES_OBSERVE_NEGBINOMIAL).xlong);
    CHECK(std::string(gft::series_op_row(gft::SERIES_LAH_ROW).x) == "p" && !gft::series_op_row(gft::SERIES_LAH_ROW).xlong);
    CHECK(&gft::series_op_row(gft::SERIES_COMPOSE_LINEAR) == &gft::SERIES_OPS[14]);
    bool threw = false;
    try {
        gft::series_op_row(gft::SERIES_OP_COUNT);
    } catch (const std::logic_error&) {
        threw = true;
    }
    CHECK(threw);
    CHECK(verdict(negbin(1, 1, 9, 1, 3, 7, batch, 1), &a).empty() && a.it.nx[2] == 9 && a.it.n[2] == 7 && a.g.items == 3);
    CHECK(verdict(negbin(1, 1, 9, 1, 7, 3, batch, 1)).empty());
    CHECK(verdict(negbin(1, 1, 9, 1, 1, 9, batch, 1)).empty());  // order 0
    expect(negbin(1, 1, 9, 1, 0, 3, batch, 1), "series_observe_negbinomial: ls holds no entry (a row of order K has K + 1 >= 1 entries)");
    expect(negbin(1, 1, 9, 1, 0, 2, batch, 1), "series_observe_negbinomial: ls holds no entry (a row of order K has K + 1 >= 1 entries)");
    for (size_t d : {2, 1, 0})
        expect(negbin(1, 1, 9, 1, 3, d, batch, 1),
               "series_observe_negbinomial: degree_p1 = " + std::to_string(d) +
                   " (the result needs at least three coefficients: degree_p1 >= 3; at two the reference multiplies by a linear power in every pass, a form "
                   "this version leaves out)");
    expect(negbin(1, 1, 9, 1, 3, 8, batch, 1),
           "series_observe_negbinomial: degree_p1 + order = 8 + 2, but a has 9 stored coefficients (every pass takes one: degree_p1 + order <= 9)");
    expect(negbin(1, 1, 9, 1, (size_t)-1, 8, batch, 1),
           "series_observe_negbinomial: degree_p1 + order = 8 + 18446744073709551614, but a has 9 stored coefficients (every pass takes one: degree_p1 + order <= 9)");
    expect(negbin(1, 1, 9, 1, 3, 10, batch, 1),
           "series_observe_negbinomial: degree_p1 + order = 10 + 2, but a has 9 stored coefficients (every pass takes one: degree_p1 + order <= 9)");
    gft::SeriesCall c = negbin(1, 1, 9, 1, 3, 7, batch, 1);
    c.r.len[2] = 6;
    expect(c, "series_observe_negbinomial: the result has 6 coefficients; with degree_p1 = 7 it has 7");
    expect(negbin(1, 1, 0, 1, 3, 7, batch, 1), "series_observe_negbinomial: a has no coefficients");
    // the family limits bound the operand and are judged before the operation's own rules; then 3 * degree_p1 + order
    expect(negbin(1, 1, 4097, 1, 0, 0, batch, 1), "series_observe_negbinomial: na = 4097 exceeds the limit of 4096 coefficients per series of this version");
    expect(negbin(1, 1, 2049, 1, 1, 3, batch, 1, 2),
           "interval series_observe_negbinomial: na = 2049 exceeds the limit of 2048 coefficients per series of this version");
    CHECK(verdict(negbin(1, 1, 2736, 1, 9, 2728, batch, 1)).empty());
    expect(negbin(1, 1, 2737, 1, 9, 2729, batch, 1),
           "series_observe_negbinomial: 3 * degree_p1 + order = 3 * 2729 + 8 exceeds the limit of 8192 of this operation (three lines of a pass lie in 64 KB of LDS)");
    const size_t single[1] = {1};
    CHECK(verdict(negbin(1, 1, 4096, 1, 4094, 3, single, 1)).empty());  // a long row on a short result: 9 + 4093
    CHECK(verdict(negbin(1, 1, 1370, 1, 9, 1362, batch, 1, 2)).empty());
    expect(negbin(1, 1, 1371, 1, 9, 1363, batch, 1, 2),
           "interval series_observe_negbinomial: 3 * degree_p1 + order = 3 * 1363 + 8 exceeds the limit of 4096 of this operation (three lines of a pass lie in 64 KB of "
           "LDS)");
    // rank 2: the axis, the lengths on it, the result's other axis cut to min(len, degree_p1)
    CHECK(verdict(negbin(2, 5, 7, 1, 3, 4, batch, 1), &a).empty() && a.it.n[1] == 4 && a.it.n[2] == 4 && a.it.xs[1] == 7);
    CHECK(verdict(negbin(2, 5, 7, 0, 3, 3, batch, 1), &a).empty() && a.it.n[1] == 3 && a.it.n[2] == 3);
    CHECK(verdict(negbin(2, 1, 9, 1, 3, 3, batch, 1), &a).empty() && a.it.n[1] == 1 && a.it.n[2] == 3);
    CHECK(verdict(negbin(2, 9, 1, 0, 7, 3, batch, 1), &a).empty() && a.it.n[1] == 3 && a.it.n[2] == 1);
    CHECK(verdict(negbin(2, 64, 64, 0, 9, 56, batch, 1)).empty());
    for (int var : {2, -1})
        expect(negbin(2, 5, 7, var, 3, 3, batch, 1),
               "series2_observe_negbinomial: var = " + std::to_string(var) + " (the variable the operation acts on is 0 or 1)");
    expect(negbin(2, 5, 7, 0, 3, 4, batch, 1),
           "series2_observe_negbinomial: degree_p1 + order = 4 + 2, but a has 5 stored coefficients on axis 0 (every pass takes one: degree_p1 + order <= 5)");
    expect(negbin(2, 5, 7, 1, 3, 2, batch, 1),
           "series2_observe_negbinomial: degree_p1 = 2 (the result needs at least three coefficients on axis 1: degree_p1 >= 3; at two the reference multiplies by a "
           "linear power in every pass, a form this version leaves out)");
    c = negbin(2, 5, 7, 1, 3, 3, batch, 1);
    c.r.len[1] = 5;
    expect(c, "series2_observe_negbinomial: the result has 5 x 3 coefficients; with degree_p1 = 3 it has 3 x 3");
    expect(negbin(2, 64, 65, 1, 3, 3, batch, 1),
           "series2_observe_negbinomial: a has 64 * 65 coefficients, which exceeds the limit of 4096 coefficients per item of this version");
    // rank 3 and BigFloat have no such operations: the pinned texts, in front of every new check (a call that breaks every new rule)
    c = negbin(2, 5, 7, 1, 0, 0, batch, 1);
    c.rank = 3, c.fn = "series3_observe_negbinomial";
    expect(c, "series3_observe_negbinomial: no such operation at rank 3 in this version (mul / div / exp / log on f64)");
    c = lah((size_t)-1, batch, 1);
    c.rank = 3, c.fn = "series3_lah_row";
    expect(c, "series3_lah_row: no such operation at rank 3 in this version (mul / div / exp / log on f64)");
    c = negbin(1, 1, 9, 1, 0, 0, batch, 1, 2);
    c.elem = gft::SERIES_ELEM_BIGFLOAT, c.fn = "bigfloat series_observe_negbinomial";
    expect(c, "bigfloat series_observe_negbinomial: no such operation on BigFloat series in this version (mul / div / exp / log / compose / pow)");
    c = lah((size_t)-1, batch, 1, 2);
    c.elem = gft::SERIES_ELEM_BIGFLOAT, c.fn = "bigfloat series_lah_row";
    expect(c, "bigfloat series_lah_row: no such operation on BigFloat series in this version (mul / div / exp / log / compose / pow)");
    // an empty batch: nothing to do, no stride looked at
    const size_t none[2] = {3, 0};
    bool ran = true;
    CHECK(verdict(negbin(1, 1, 9, 1, 3, 7, none, 2), nullptr, &ran).empty() && !ran);
}

static void scalars() {
    const size_t batch[2] = {3, 2};
    gft::SeriesArgs a;
    // null stride arrays: contiguous items; x and p one per item, ls nls per item -- the batch collapses to one axis
    CHECK(verdict(negbin(1, 1, 9, 1, 3, 7, batch, 2), &a).empty());
    CHECK(a.g.nd == 1 && a.g.ext[0] == 6 && a.g.xs[0] == 9 && a.g.ys[0] == 1 && a.ps[0] == 1 && a.g.ss[0] == 3 && a.g.rs[0] == 7 && a.pp == 0);
    // stride 0 on p alone keeps the axes apart: p's strides are part of the collapse
    const int64_t p0[2] = {0, 1}, x0[2] = {0, 0}, l0[2] = {0, 3};
    gft::SeriesCall c = negbin(1, 1, 9, 1, 3, 7, batch, 2);
    c.p.bs = p0;
    CHECK(verdict(c, &a).empty() && a.g.nd == 2 && a.ps[0] == 0 && a.ps[1] == 1 && a.g.ys[0] == 2 && a.g.ys[1] == 1);
    c.y.bs = x0, c.cs.bs = l0;
    CHECK(verdict(c, &a).empty() && a.g.nd == 2 && a.g.ys[0] == 0 && a.g.ys[1] == 0 && a.g.ss[0] == 0 && a.g.ss[1] == 3 && a.ps[1] == 1);
    // x and p are required
    c = negbin(1, 1, 9, 1, 3, 7, batch, 2);
    bool null_x = false, null_p = false;
    try {
        gft::SeriesArgs s;
        c.y.p = nullptr;
        gft::series_args(c, s, [&](const double* q, const char* what) { null_x = null_x || (!q && std::string(what) == "x"); });
        c = negbin(1, 1, 9, 1, 3, 7, batch, 2);
        c.p.p = nullptr;
        gft::series_args(c, s, [&](const double* q, const char* what) { null_p = null_p || (!q && std::string(what) == "p"); });
    } catch (const std::exception&) {
    }
    CHECK(null_x && null_p);  // (the caller's pointer check is handed both, null as they are)
    // intervals: the plane stride leads every array; null arrays are planes back to back
    CHECK(verdict(negbin(1, 1, 9, 1, 3, 7, batch, 2, 2), &a).empty());
    CHECK(a.pl.x == 54 && a.pl.y == 6 && a.pp == 6 && a.pl.s == 18 && a.pl.r == 42);
    const int64_t pp[3] = {0, 2, 1};  // point scalars
    c = negbin(1, 1, 9, 1, 3, 7, batch, 2, 2);
    c.p.bs = pp;
    CHECK(verdict(c, &a).empty() && a.pp == 0 && a.ps[0] == 1 && a.pl.y == 6);
    const int64_t neg[2] = {-2, 1};
    c = negbin(1, 1, 9, 1, 3, 7, batch, 2);
    c.p.bs = neg;
    expect(c, "series_observe_negbinomial: negative strides are not supported (p, batch axis 0)");
    c = negbin(1, 1, 9, 1, 3, 7, batch, 2);
    c.cs.bs = neg;
    expect(c, "series_observe_negbinomial: negative strides are not supported (ls, batch axis 0)");
}

static void overlaps() {
    const size_t batch[1] = {3};
    gft::SeriesCall c = negbin(1, 1, 9, 1, 3, 7, batch, 1);
    c.r.p = buffer + 1;
    expect(c, "series_observe_negbinomial: the result partially overlaps a (it may alias an operand only as the same view)");
    c.r.p = buffer;
    expect(c, "series_observe_negbinomial: the result partially overlaps a (it may alias an operand only as the same view)");
    c = negbin(1, 1, 9, 1, 3, 7, batch, 1);
    c.y.p = buffer + 32768 + 20;
    expect(c, "series_observe_negbinomial: the result partially overlaps x (it may alias an operand only as the same view)");
    c = negbin(1, 1, 9, 1, 3, 7, batch, 1);
    c.p.p = buffer + 32768 + 20;
    expect(c, "series_observe_negbinomial: the result partially overlaps p (it may alias an operand only as the same view)");
    c.p.p = buffer + 32768 + 21;  // just behind the result's last element
    CHECK(verdict(c).empty());
    c = negbin(1, 1, 9, 1, 3, 7, batch, 1);
    c.cs.p = buffer + 32768 + 18;
    expect(c, "series_observe_negbinomial: the result partially overlaps ls (it may alias an operand only as the same view)");
    const int64_t zero[1] = {0};
    c = negbin(1, 1, 9, 1, 3, 7, batch, 1);
    c.r.bs = zero;
    expect(c, "series_observe_negbinomial: the result has a zero stride (batch axis 0): its series overlap");
}

static void lah_rows() {
    const size_t batch[2] = {3, 2};
    gft::SeriesArgs a;
    CHECK(verdict(lah(0, batch, 2), &a).empty() && a.g.nd == 1 && a.g.ext[0] == 6 && a.g.xs[0] == 1 && a.g.rs[0] == 1 && a.it.n[2] == 1);
    CHECK(verdict(lah(7, batch, 2), &a).empty() && a.g.nd == 1 && a.g.xs[0] == 1 && a.g.rs[0] == 8 && a.it.n[2] == 8 && a.it.nx[2] == 1);
    CHECK(verdict(lah(4095, batch, 2)).empty());
    expect(lah(4096, batch, 2), "series_lah_row: order + 1 = 4097 exceeds the limit of 4096 coefficients per series of this version");
    expect(lah((size_t)-1, batch, 2), "series_lah_row: order + 1 = 2^64 exceeds the limit of 4096 coefficients per series of this version");
    CHECK(verdict(lah(2047, batch, 2, 2), &a).empty() && a.pl.x == 6 && a.pl.r == 6 * 2048);
    expect(lah(2048, batch, 2, 2), "interval series_lah_row: order + 1 = 2049 exceeds the limit of 2048 coefficients per series of this version");
    const int64_t p0[2] = {0, 0};  // one p for every item
    gft::SeriesCall c = lah(7, batch, 2);
    c.x.bs = p0;
    CHECK(verdict(c, &a).empty() && a.g.nd == 1 && a.g.xs[0] == 0 && a.g.rs[0] == 8);
    c = lah(7, batch, 2);
    c.x.p = buffer + 32768 + 47;  // the last element of the last row
    expect(c, "series_lah_row: the result partially overlaps p (it may alias an operand only as the same view)");
    c.x.p = buffer + 32768;  // a row may not start on its own p either: never "the same view"
    expect(c, "series_lah_row: the result partially overlaps p (it may alias an operand only as the same view)");
    const int64_t neg[2] = {-1, 1};
    c = lah(7, batch, 2);
    c.x.bs = neg;
    expect(c, "series_lah_row: negative strides are not supported (p, batch axis 0)");
}

int main() {
    rules();
    scalars();
    overlaps();
    lah_rows();
    if (failures) {
        std::printf("FAILED %ld of %ld checks\n", failures, checks);
        return 1;
    }
    std::printf("ok %ld checks\n", checks);
    return 0;
}
