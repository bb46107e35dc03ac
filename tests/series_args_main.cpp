// The host-side argument layer of the batched series calls (genfer_amd/csrc/gft_series_args.hpp) on its own: no HIP, no device.
// Reads one call per line on stdin (test_series_refusals.py writes them from tests/series_refusals.json) and prints one line per
// call: "E <message>" for a refusal, "EMPTY" for an empty batch, else the collapsed batch and the plane strides.
//   op w rank2 e var k  nbatch|null b...  <x> <y> <r>  : fn
//   a view is  off|null  nbs|null s...  rst len0 len1      (off: doubles into one buffer that is never read)
// With the argument "ops" it reads nothing and prints the table of the operations, one row of gft::SERIES_OPS per line (names "|"-separated).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../genfer_amd/csrc/gft_series_args.hpp"

static double buffer[8192 + 256];  // make_series_refusals.py BUFFER

struct View {
    gft::SeriesView v;
    std::vector<int64_t> bs;
};

static bool count(std::istream& in, size_t& n) {  // "null" or a count
    std::string t;
    in >> t;
    if (t == "null") return false;
    n = std::stoull(t);
    return true;
}

static void read_view(std::istream& in, View& w) {
    size_t off = 0, nbs = 0;
    w.v.p = count(in, off) ? buffer + off : nullptr;
    const bool has = count(in, nbs);
    w.bs.resize(nbs);
    for (auto& s : w.bs) in >> s;
    in >> w.v.st[1] >> w.v.len[1] >> w.v.len[2];
    w.v.bs = has ? w.bs.data() : nullptr;
}

template <class T>
static void list(const char* name, const T* a, int n) {
    std::printf(" %s=[", name);
    for (int i = 0; i < n; ++i) std::printf(i ? ",%zu" : "%zu", (size_t)a[i]);
    std::printf("]");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "ops") {  // the rows of gft::SERIES_OPS: index family ranks long x y cs
        const char* const family[] = {"arith", "pow", "observe", "chain", "linear"};
        for (const gft::SeriesOpRow& r : gft::SERIES_OPS)
            std::printf("%d %s %d %s %s|%s|%s\n", (int)r.op, family[r.family], r.ranks, r.xlong ? "x" : "result", r.x, r.y, r.cs);
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        gft::SeriesCall c;
        int rank2 = 0;
        in >> c.op >> c.w >> rank2 >> c.e >> c.var >> c.k;
        c.rank = rank2 ? 2 : 1;
        std::vector<size_t> batch;
        const bool has_batch = count(in, c.nbatch);
        batch.resize(has_batch ? c.nbatch : 0);
        for (auto& b : batch) in >> b;
        if (!has_batch) in >> c.nbatch;  // a null batch still states how many axes it claims
        c.batch = has_batch ? batch.data() : nullptr;
        View x, y, r;
        read_view(in, x), read_view(in, y), read_view(in, r);
        c.x = x.v, c.y = y.v, c.r = r.v;
        std::string colon, fn;
        in >> colon;
        std::getline(in, fn);
        fn.erase(0, fn.find_first_not_of(' '));
        c.fn = fn.c_str();
        if (!in || colon != ":") {
            std::printf("BAD LINE %s\n", line.c_str());
            return 2;
        }
        try {
            gft::SeriesArgs a;
            if (!gft::series_args(c, a, [](const double*, const char*) {})) {  // the pointer check needs the device: not here
                std::printf("EMPTY\n");
                continue;
            }
            const gft::SeriesBatch& g = a.g;
            std::printf("OK nd=%d items=%u inplace=%d", g.nd, g.items, g.inplace);
            list("ext", g.ext, g.nd), list("xs", g.xs, g.nd), list("ys", g.ys, g.nd), list("ss", g.ss, g.nd), list("rs", g.rs, g.nd);
            std::printf(" planes=%d,%zu,%zu,%zu,%zu rows=%zu,%zu,%zu\n", a.pl.w, a.pl.x, a.pl.y, a.pl.s, a.pl.r, a.it.xs[1], a.it.ys[1], a.it.rs[1]);
        } catch (const std::exception& e) {
            std::printf("E %s\n", e.what());
        }
    }
    return 0;
}
