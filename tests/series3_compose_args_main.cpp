// compose and pow at rank 3 in the host-side argument layer (genfer_amd/csrc/gft_series_args.hpp) on their own: no HIP, no device.
// A self-checking program (tests/test_series3_compose_cpu.py builds and runs it; exit status 0 and a line of counts when all holds):
//   * over every f, g and n with 1 .. 3 coefficients per axis and every var: series3_compose_dims' final stored shape against the loop
//     of the definition walked here, the permutation (unit axes of S in front, the others in order), the permuted position of var, the
//     permuted shapes and strides, the caller-order full / keep / fs of the padding -- and, step by step, that the Series3Dims of the
//     step's product mul3(res, g, L) (series3_product_dims) has the SAME permutation: one serves the whole loop;
//   * over the same grid the verdict of series_args: accepted iff nf, ng <= n per axis, else the refusal's exact text;
//   * the other refusals by name: var, the limit, empty shapes, strides, overlaps through the slab axis, pow's batch axes;
//   * pow's chain of compact shapes through series3_compact / series3_product_dims at a few exponents.
#include <cstdio>
#include <string>
#include <vector>

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

static gft::SeriesView view(size_t off, const unsigned* s, const int64_t* bs = nullptr, int64_t sst = -1, int64_t rst = -1) {
    gft::SeriesView v;
    v.p = buffer + off, v.bs = bs;
    v.len[0] = s[0], v.len[1] = s[1], v.len[2] = s[2];
    v.st[0] = sst >= 0 ? sst : (int64_t)(s[1] * s[2]), v.st[1] = rst >= 0 ? rst : (int64_t)s[2];
    return v;
}

// "" for an accepted call, else the message
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

static gft::SeriesCall compose_call(const unsigned* nf, const unsigned* ng, const unsigned* n, int var, const size_t* batch, size_t nbatch) {
    gft::SeriesCall c;
    c.op = gft::SERIES_COMPOSE, c.fn = "series3_compose", c.rank = 3, c.var = var, c.batch = batch, c.nbatch = nbatch;
    c.x = view(0, nf), c.y = view(8192, ng), c.r = view(16384, n);
    return c;
}

static std::string dims(const unsigned* s) { return std::to_string(s[0]) + " x " + std::to_string(s[1]) + " x " + std::to_string(s[2]); }

static void grid() {
    const size_t batch[1] = {3};
    unsigned nf[3], ng[3], n[3];
    for (unsigned code = 0; code < 19683; ++code) {  // 3^9: every shape of f, g and n with 1 .. 3 coefficients per axis
        unsigned q = code;
        for (int a = 0; a < 3; ++a) nf[a] = 1 + q % 3, q /= 3;
        for (int a = 0; a < 3; ++a) ng[a] = 1 + q % 3, q /= 3;
        for (int a = 0; a < 3; ++a) n[a] = 1 + q % 3, q /= 3;
        bool f_fits = true, g_fits = true;
        for (int a = 0; a < 3; ++a) f_fits = f_fits && nf[a] <= n[a], g_fits = g_fits && ng[a] <= n[a];
        for (int var = 0; var < 3; ++var) {
            gft::SeriesArgs args;
            const std::string got = verdict(compose_call(nf, ng, n, var, batch, 1), &args);
            if (!f_fits || !g_fits) {
                const std::string want = std::string("series3_compose: ") + (f_fits ? "g" : "f") + " has " + dims(f_fits ? ng : nf) +
                                         " coefficients, the result " + dims(n) + " (an operand is longer than the truncation order)";
                CHECK(got == want);
                continue;
            }
            CHECK(got.empty());
            if (!got.empty()) continue;
            const gft::Series3Compose k = gft::series3_compose_dims(args.it, var);
            // the definition's loop, in the caller's order
            unsigned r[3] = {nf[0], nf[1], nf[2]}, L[3];
            r[var] = 1;
            std::vector<std::vector<unsigned>> steps;
            for (unsigned i = 0; i + 1 < nf[var]; ++i) {
                for (int a = 0; a < 3; ++a) L[a] = std::min(r[a] + ng[a] - 1, n[a]);
                steps.push_back({r[0], r[1], r[2], L[0], L[1], L[2]});
                for (int a = 0; a < 3; ++a) r[a] = L[a];
            }
            int order[3], m = 0;
            for (int a = 0; a < 3; ++a)
                if (r[a] == 1) order[m++] = a;
            for (int a = 0; a < 3; ++a)
                if (r[a] != 1) order[m++] = a;
            const size_t fst[3] = {(size_t)nf[1] * nf[2], nf[2], 1}, gst[3] = {(size_t)ng[1] * ng[2], ng[2], 1}, rst[3] = {(size_t)n[1] * n[2], n[2], 1};
            // (the argument layer states the stride of an axis of one coefficient as 0, the unit-stride axis always as 1)
            auto stride = [](const unsigned* shape, const size_t* st, int o) { return o == 2 ? (size_t)1 : (shape[o] > 1 ? st[o] : (size_t)0); };
            for (int i = 0; i < 3; ++i) {
                const int o = order[i];
                CHECK(k.keep[i] == r[i] && k.full[i] == n[i] && k.fs[i] == stride(n, rst, i));
                CHECK(k.s[i] == r[o] && k.n[i] == n[o] && k.ng[i] == ng[o] && k.sl[i] == (o == var ? 1u : nf[o]));
                CHECK(k.xs[i] == stride(nf, fst, o) && k.ys[i] == stride(ng, gst, o) && k.rs[i] == stride(n, rst, o));
                if (o == var) CHECK(k.var == i);
            }
            CHECK(k.slices == nf[var] && k.fslice == stride(nf, fst, var));
            // every step's product is series3.mul's: its stored shape is L, and its permuted item is the loop's permuted item
            for (const auto& s : steps) {
                const gft::Series3Dims p = gft::series3_product_dims(&s[0], ng, &s[3]);
                for (int i = 0; i < 3; ++i) {
                    const int o = order[i];
                    CHECK(p.keep[i] == s[3 + i]);                                      // S of the step is L itself
                    CHECK(p.n[i] == s[3 + o] && p.nx[i] == s[o] && p.ny[i] == ng[o]);  // the same permutation at every step
                    CHECK((s[3 + i] == 1) == (r[i] == 1));                             // the unit axes of a step are those of the final shape
                }
            }
        }
    }
}

static void expect(const gft::SeriesCall& c, const char* want) {
    const std::string got = verdict(c);
    ++checks;
    if (got != want) {
        if (++failures <= 20) std::printf("FAILED: want \"%s\"\n        got  \"%s\"\n", want, got.c_str());
    }
}

static void refusals() {
    const size_t batch[1] = {3};
    const unsigned N[3] = {2, 3, 4}, big[3] = {17, 241, 1}, zero[3] = {2, 0, 4};
    for (int var : {3, -1, 7}) {
        const std::string want = "series3_compose: var = " + std::to_string(var) + " (the variable of f that g replaces is 0, 1 or 2)";
        expect(compose_call(N, N, N, var, batch, 1), want.c_str());
    }
    expect(compose_call(N, N, big, 0, batch, 1), "series3_compose: n0 * n1 * n2 = 17 * 241 * 1 exceeds the limit of 4096 coefficients per item of this version");
    expect(compose_call(N, N, zero, 0, batch, 1), "series3_compose: n0 * n1 * n2 == 0 (the result has no coefficients)");
    expect(compose_call(zero, N, N, 0, batch, 1), "series3_compose: an operand has no coefficients");
    expect(compose_call(N, zero, N, 0, batch, 1), "series3_compose: an operand has no coefficients");
    gft::SeriesCall c = compose_call(N, N, N, 1, batch, 1);
    c.x.st[0] = -12;
    expect(c, "series3_compose: negative strides are not supported (f, the slab axis)");
    c = compose_call(N, N, N, 1, batch, 1);
    c.y.st[1] = -4;
    expect(c, "series3_compose: negative strides are not supported (g, the row axis)");
    c = compose_call(N, N, N, 1, batch, 1);
    c.r.st[0] = 0;
    expect(c, "series3_compose: the result has a zero slab stride: the slabs of an item overlap");
    c = compose_call(N, N, N, 1, batch, 1);
    c.r.st[0] = 8;
    expect(c, "series3_compose: the result's series overlap each other (its strides do not separate the rows)");
    // the slab axis in the overlap proof: a result one slab into f, and one that differs from g by its slab stride alone
    c = compose_call(N, N, N, 2, batch, 1);
    c.r.p = c.x.p + 12;
    expect(c, "series3_compose: the result partially overlaps f (it may alias an operand only as the same view)");
    const int64_t wide[1] = {40};
    c = compose_call(N, N, N, 2, batch, 1);
    c.y = view(8192, N, wide, 16), c.r = view(8192, N, wide, 12);
    expect(c, "series3_compose: the result partially overlaps g (it may alias an operand only as the same view)");
    // the same view is accepted, on either operand, and says so
    gft::SeriesArgs a;
    c = compose_call(N, N, N, 2, batch, 1);
    c.r = c.x;
    CHECK(verdict(c, &a).empty() && a.g.inplace == 1);
    c = compose_call(N, N, N, 2, batch, 1);
    c.y = view(8192, N, wide, 16), c.r = c.y;
    CHECK(verdict(c, &a).empty() && a.g.inplace == 1);
    // pow: admitted at rank 3, no second operand; the copy carries the batch axes, the slabs, the rows and the series
    gft::SeriesCall p;
    p.op = gft::SERIES_POW, p.fn = "series3_pow", p.rank = 3, p.e = 5, p.batch = batch, p.nbatch = 1;
    p.x = view(0, N), p.r = view(16384, N);
    CHECK(verdict(p, &a).empty() && a.g.inplace == 0 && a.g.items == 3);
    p.r = p.x;
    CHECK(verdict(p, &a).empty() && a.g.inplace == 1);
    p.r = view(4, N);
    expect(p, "series3_pow: the result partially overlaps x (it may alias an operand only as the same view)");
    const unsigned longer[3] = {2, 3, 5};
    p.x = view(0, longer), p.r = view(16384, N);
    expect(p, "series3_pow: x has 2 x 3 x 5 coefficients, the result 2 x 3 x 4 (an operand is longer than the truncation order)");
    {
        // 11 batch axes of 2, none contiguous with its neighbour on x (its strides alternate between 24 and 0; the result is
        // contiguous): one more than the copy can carry beside the three series axes
        size_t b11[11];
        int64_t xbs[11], rbs[11];
        int64_t rs = 24;
        for (int i = 10; i >= 0; --i) b11[i] = 2, xbs[i] = i % 2 ? 0 : 24, rbs[i] = rs, rs *= 2;
        gft::SeriesCall q = p;
        q.batch = b11, q.nbatch = 11;
        q.x = view(0, N, xbs), q.r = view(16384, N, rbs);  // (2^11 items of 24: the result ends where the buffer does)
        expect(q, "series3_pow: the batch has more than 10 non-contiguous axes");
        q.batch = b11 + 1, q.nbatch = 10, q.x.bs = xbs + 1, q.r.bs = rbs + 1;
        CHECK(verdict(q, &a).empty() && a.g.nd == 10);
    }
    // an operation that rank 3 does not have keeps its text
    gft::SeriesCall t = compose_call(N, N, N, 0, batch, 1);
    t.op = gft::SERIES_CORR, t.fn = "series3_corr";
    expect(t, "series3_corr: no such operation at rank 3 in this version (mul / div / exp / log on f64)");
}

static void pow_chain() {
    // x of (2, 1, 3) under n = (4, 2, 5), e = 5 = 0b101: res = 1 * x; base = x^2; base = x^4; res = x * x^4
    const unsigned n[3] = {4, 2, 5}, x[3] = {2, 1, 3}, one[3] = {1, 1, 1};
    unsigned L[3];
    gft::series3_compact(one, x, n, L);
    CHECK(L[0] == 2 && L[1] == 1 && L[2] == 3);
    gft::Series3Dims d = gft::series3_product_dims(one, x, L);
    CHECK(d.keep[0] == 2 && d.keep[1] == 1 && d.keep[2] == 3 && d.n[0] == 1 && d.n[1] == 2 && d.n[2] == 3);  // the unit axis in front
    CHECK(d.ny[0] == 1 && d.ny[1] == 2 && d.ny[2] == 3 && d.ys[0] == 3 && d.ys[1] == 3 && d.ys[2] == 1 && d.rs[1] == 3 && d.rs[2] == 1);
    unsigned b2[3], b4[3], last[3];
    gft::series3_compact(x, x, n, b2);
    CHECK(b2[0] == 3 && b2[1] == 1 && b2[2] == 5);
    gft::series3_compact(b2, b2, n, b4);
    CHECK(b4[0] == 4 && b4[1] == 1 && b4[2] == 5);
    gft::series3_compact(x, b4, n, last);
    CHECK(last[0] == 4 && last[1] == 1 && last[2] == 5);
    // the last product writes all of n through the result's strides; what lies outside S = (4, 1, 5) is the zero fill's
    const size_t rs[3] = {100, 10, 1};
    d = gft::series3_product_dims(x, b4, n, rs);
    CHECK(d.full[1] == 2 && d.keep[1] == 1 && d.fs[0] == 100 && d.fs[1] == 10 && d.n[0] == 1 && d.n[1] == 4 && d.n[2] == 5);
    CHECK(d.rs[0] == 10 && d.rs[1] == 100 && d.rs[2] == 1);
}

int main() {
    grid();
    refusals();
    pow_chain();
    std::printf("%s checks=%ld failures=%ld\n", failures ? "FAILED" : "OK", checks, failures);
    return failures ? 1 : 0;
}
