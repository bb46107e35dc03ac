// The row-pair planner (genfer_amd/csrc/gft_pair_plan.hpp) checked without a device, two ways.
// (a) Against tests/golden/pair_plan_table.txt: one case per line, inputs then the plan, every field of every range.  The table
//     was printed by the planning code as it stood inside the launcher before the planner was split out; a change to it is a
//     change of what runs, not a refactor.
// (b) In itself, by brute force, for every accepted case of at most ~10^5 output rows: the ranges tile the leading axes, their
//     slots chain and fit the cap, and the phase-1 grid is exact — every workgroup index decodes (as k_pair_sums decodes it) to a
//     distinct valid combination, and every (x row, y row) pair of the range is computed by exactly one lane, into its own slot.
// Usage: pair_plan_check <table>.  Built and run by tests/test_pair_plan.py.
#include <cstdio>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "gft_pair_plan.hpp"

using namespace gft;
typedef unsigned long long u64;

struct Case {
    int W, nd, slack, lanes, avail;
    unsigned xs[4], ys[4], zs[4];
    size_t xstr[4], ystr[4], zstr[4];
    size_t cap;
    PairShape shape() const { return PairShape{nd, xs, ys, zs, xstr, ystr, zstr, slack != 0}; }
};

static std::string inputs(const Case& c) {
    std::ostringstream o;
    o << c.W << ' ' << c.nd;
    for (const unsigned* v : {c.xs, c.ys, c.zs})
        for (int i = 0; i < c.nd; ++i) o << ' ' << v[i];
    o << ' ' << c.slack << ' ' << c.cap << ' ' << c.lanes << ' ' << c.avail;
    return o.str();
}

static std::string dump(bool ok, const PairPlan& p) {
    std::ostringstream o;
    o << "=> " << (ok ? 1 : 0);
    if (!ok) return o.str();
    o << ' ' << (p.use_lanes ? 1 : 0) << ' ' << p.size() << ' ' << p.most << ' ' << p.lds;
    for (size_t i = 0; i < p.size(); ++i) {
        const PairRange& r = p[i];
        const PairArgs& q = r.args;
        o << " ; " << r.lo << ' ' << r.hi << ' ' << r.band << ' ' << r.ku << ' ' << r.base << ' ' << r.slots << ' ' << r.nwg << ' ' << r.nrows;
        for (unsigned v : {q.xU, q.x0, q.x1, q.yU, q.y0, q.y1, q.zU, q.z0, q.z1, q.n2, q.nx2, q.n8, q.nb, q.nxc, q.tsh, q.NW, q.xch, q.tiles0, q.tiles1, q.pitch})
            o << ' ' << v;
        o << ' ' << q.S0 << ' ' << q.S1 << ' ' << q.band << ' ' << q.klo << ' ' << q.khi << ' ' << q.slot_base << ' ' << q.c1tot << ' ' << q.s0tot << ' '
          << q.at_lo << ' ' << q.kuf;
    }
    return o.str();
}

static bool parse(const std::string& line, Case& c, std::string& want) {
    std::istringstream in(line);
    if (!(in >> c.W >> c.nd) || c.nd < 1 || c.nd > 4) return false;
    for (unsigned* v : {c.xs, c.ys, c.zs})
        for (int i = 0; i < c.nd; ++i)
            if (!(in >> v[i])) return false;
    if (!(in >> c.slack >> c.cap >> c.lanes >> c.avail)) return false;
    size_t sx = 1, sy = 1, sz = 1;
    for (int i = c.nd - 1; i >= 0; --i) {
        c.xstr[i] = sx, c.ystr[i] = sy, c.zstr[i] = sz;
        sx *= c.xs[i], sy *= c.ys[i], sz *= c.zs[i];
    }
    const size_t at = line.find("=>");
    if (at == std::string::npos) return false;
    want = line.substr(at);
    return true;
}

// ---- (b)

static int fails = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            if (fails++ < 20) {                       \
                std::printf("FAIL %s: ", what.c_str()); \
                std::printf(__VA_ARGS__);             \
                std::printf("\n");                    \
            }                                         \
            return;                                   \
        }                                             \
    } while (0)

// k_pair_sums' slot of the row sum of x row (ju, j0, j1) with the y row that takes it to output row (ku, k0, k1)
static u64 pair_slot(const PairArgs& g, unsigned ju, unsigned j0, unsigned j1, unsigned ku, unsigned k0, unsigned k1) {
    const unsigned cU = pair_cnt(ku, g.xU, g.yU), c0 = pair_cnt(k0, g.x0, g.y0), c1 = pair_cnt(k1, g.x1, g.y1);
    const u64 base = pair_pre(ku, g.xU, g.yU) * g.S0 * g.S1 + (u64)cU * (pair_pre(k0, g.x0, g.y0) * g.S1 + (u64)c0 * pair_pre(k1, g.x1, g.y1));
    return base + ((u64)(ju - pair_lo(ku, g.yU)) * c0 + (j0 - pair_lo(k0, g.y0))) * c1 + (j1 - pair_lo(k1, g.y1));
}

static bool in_range(const PairRange& r, unsigned ku, unsigned k0) {
    return r.band == 0 || (r.band == 2 && ku >= r.lo && ku < r.hi) || (r.band == 1 && ku == r.ku && k0 >= r.lo && k0 < r.hi);
}

// The range's output rows in row-major order, each row's terms in the reference's order (outer axes lexicographic, ascending
// j): their slots count up from slot_base without a gap, to `slots`; the rows are `nrows`.
static void check_slots(const std::string& what, const PairRange& r) {
    const PairArgs& g = r.args;
    u64 next = 0, rows = 0;
    for (unsigned ku = 0; ku < g.zU; ++ku)
        for (unsigned k0 = 0; k0 < g.z0; ++k0) {
            if (!in_range(r, ku, k0)) continue;
            for (unsigned k1 = 0; k1 < g.z1; ++k1, ++rows)
                for (unsigned ju = 0; ju <= ku && ju < g.xU; ++ju)
                    for (unsigned j0 = 0; j0 <= k0 && j0 < g.x0; ++j0)
                        for (unsigned j1 = 0; j1 <= k1 && j1 < g.x1; ++j1) {
                            if (ku - ju >= g.yU || k0 - j0 >= g.y0 || k1 - j1 >= g.y1) continue;
                            const u64 s = pair_slot(g, ju, j0, j1, ku, k0, k1);
                            CHECK(s >= g.slot_base && s - g.slot_base == next, "slot %llu of x (%u %u %u) -> z (%u %u %u), expected %llu + %llu", s, ju, j0,
                                  j1, ku, k0, k1, g.slot_base, next);
                            ++next;
                        }
        }
    CHECK(next == r.slots, "%llu terms, %llu slots", next, r.slots);
    CHECK(rows == r.nrows, "%llu output rows, nrows %u", rows, r.nrows);
}

// Every workgroup index of the phase-1 grid, decoded as the first lines of k_pair_sums decode blockIdx.x.
static void check_grid(const std::string& what, const PairRange& r) {
    const PairArgs& g = r.args;
    const unsigned T1 = 1u << g.tsh, T0 = 64u >> g.tsh;
    std::vector<unsigned char> hit(r.slots, 0);
    std::set<std::tuple<unsigned, unsigned, unsigned, unsigned, unsigned, unsigned>> seen;
    CHECK(g.c1tot > 0 && (g.band == 1 ? g.tiles0 > g.at_lo : g.s0tot > 0), "empty grid factors");
    for (u64 L = 0; L < r.nwg; ++L) {
        unsigned c = (unsigned)(L % g.c1tot);
        const u64 q = L / g.c1tot;
        unsigned bt = 0, n1 = 0, nc = 0;
        for (;; ++bt) {
            n1 = g.z1 - T1 * bt < g.x1 ? g.z1 - T1 * bt : g.x1;
            nc = (n1 + g.xch - 1) / g.xch;
            if (c < nc || bt + 1 >= g.tiles1) break;
            c -= nc;
        }
        CHECK(c < nc && T1 * bt < g.z1, "workgroup %llu: chunk %u of %u in tile %u of axis 1", L, c, nc, bt);
        unsigned at = 0, ud = 0, j0 = 0, ju = 0;
        if (g.band == 1) {
            const unsigned nat = g.tiles0 - g.at_lo;
            at = g.at_lo + (unsigned)(q % nat);
            j0 = at;
            ud = (g.kuf + 1 > g.xU ? g.kuf + 1 - g.xU : 0u) + (unsigned)(q / nat);
            CHECK(ud <= g.kuf && ud < g.yU, "workgroup %llu: y slab %u", L, ud);
            ju = g.kuf - ud;
        } else {
            unsigned q0 = (unsigned)(q % g.s0tot), n0 = 0, nU = 0;
            u64 qu = q / g.s0tot;
            for (;; ++at) {
                n0 = g.z0 - T0 * at < g.x0 ? g.z0 - T0 * at : g.x0;
                if (q0 < n0 || at + 1 >= g.tiles0) break;
                q0 -= n0;
            }
            CHECK(q0 < n0 && T0 * at < g.z0, "workgroup %llu: j0 %u of %u in tile %u of axis 0", L, q0, n0, at);
            j0 = q0;
            for (;; ++ud) {
                unsigned ju_lo = 0;
                nU = g.zU - ud < g.xU ? g.zU - ud : g.xU;
                if (g.band == 2) {
                    ju_lo = g.klo > ud ? g.klo - ud : 0u;
                    const unsigned hi = g.khi > ud ? (g.khi - ud < nU ? g.khi - ud : nU) : 0u;
                    nU = hi > ju_lo ? hi - ju_lo : 0u;
                }
                if (qu < nU || ud + 1 >= g.yU) {
                    ju = ju_lo + (unsigned)qu;
                    break;
                }
                qu -= nU;
            }
            CHECK(qu < nU && ud < g.zU, "workgroup %llu: x slab %llu of %u against y slab %u", L, qu, nU, ud);
        }
        CHECK(ju < g.xU && j0 < g.x0 && ud < g.yU, "workgroup %llu: x rows (%u %u), y slab %u", L, ju, j0, ud);
        CHECK(seen.insert(std::make_tuple(ju, j0, c, ud, at, bt)).second, "workgroup %llu repeats (ju %u j0 %u chunk %u ud %u at %u bt %u)", L, ju, j0, c, ud,
              at, bt);
        const int d0b = g.band == 1 ? (int)g.klo - (int)at : (int)(T0 * at);
        const unsigned d1b = T1 * bt, j1_lo = c * g.xch;
        const unsigned rows_here = j1_lo + g.xch < n1 ? g.xch : n1 - j1_lo;
        CHECK(rows_here >= 1 && rows_here <= g.xch, "workgroup %llu: %u x rows", L, rows_here);
        unsigned sums = 0;
        for (unsigned row = 0; row < rows_here; ++row)
            for (unsigned lane = 0; lane < 64; ++lane) {
                const unsigned j1 = j1_lo + row, l0 = lane >> g.tsh, l1 = lane & (T1 - 1u);
                const unsigned d0 = (unsigned)(d0b + (int)l0), d1 = d1b + l1;
                const bool row_ok = d0 < g.y0 && d1 < g.y1 && (g.band != 1 || l0 < g.khi - g.klo);
                if (!(row_ok && j0 + d0 < g.z0 && j1 + d1 < g.z1)) continue;
                CHECK(j1 < g.x1 && ju + ud < g.zU && in_range(r, ju + ud, j0 + d0), "workgroup %llu lane %u: x (%u %u %u) y (%u %u %u) outside the range", L,
                      lane, ju, j0, j1, ud, d0, d1);
                const u64 s = pair_slot(g, ju, j0, j1, ju + ud, j0 + d0, j1 + d1);
                CHECK(s >= g.slot_base && s - g.slot_base < r.slots, "workgroup %llu lane %u: slot %llu outside [%llu, +%llu)", L, lane, s, g.slot_base, r.slots);
                CHECK(hit[s - g.slot_base]++ == 0, "workgroup %llu lane %u: x (%u %u %u) y (%u %u %u) computed twice", L, lane, ju, j0, j1, ud, d0, d1);
                ++sums;
            }
        CHECK(sums > 0, "workgroup %llu (ju %u j0 %u chunk %u ud %u at %u bt %u) has no row sum to compute", L, ju, j0, c, ud, at, bt);
    }
    // (check_slots: the range's slots are its (x row, y row) pairs, one each)
    for (u64 s = 0; s < r.slots; ++s) CHECK(hit[s] == 1, "slot %llu + %llu: no workgroup computes it", g.slot_base, s);
}

static void check_plan(const std::string& what, const Case& c, const PairPlan& p) {
    const PairArgs& g = p[0].args;
    const u64 row_bytes = (u64)g.n2 * c.W * sizeof(double), total = pair_pre(g.zU, g.xU, g.yU) * g.S0 * g.S1;
    std::vector<unsigned> cover((size_t)g.zU * g.z0, 0);
    u64 next = 0, most = 0;
    CHECK(!p.use_lanes || (p.size() >= 2 && c.avail && c.lanes != 0), "two lanes for %zu ranges (mode %d, available %d)", p.size(), c.lanes, c.avail);
    for (size_t i = 0; i < p.size(); ++i) {
        const PairRange& r = p[i];
        CHECK(r.band <= 2 && (r.band == 0 ? p.size() == 1 : r.lo < r.hi), "range %zu: band %u [%u, %u)", i, r.band, r.lo, r.hi);
        for (unsigned ku = 0; ku < g.zU; ++ku)
            for (unsigned k0 = 0; k0 < g.z0; ++k0) cover[(size_t)ku * g.z0 + k0] += in_range(r, ku, k0);
        CHECK(r.base == next && r.args.slot_base == r.base, "range %zu starts at slot %llu, the one before ends at %llu", i, r.base, next);
        next += r.slots;
        CHECK(r.slots * row_bytes <= (p.use_lanes ? c.cap / 2 : c.cap), "range %zu: %llu bytes of row sums", i, r.slots * row_bytes);
        most = std::max(most, r.slots * row_bytes);
        CHECK(r.nwg >= 1 && r.nwg <= 0x7fffffffu && r.nrows >= 1 && r.nrows <= 0x7fffffffu, "range %zu: grids %u, %u", i, r.nwg, r.nrows);
        CHECK(r.band != 1 || r.hi - r.lo <= (64u >> r.args.tsh), "range %zu: %u slabs in a window of %u", i, r.hi - r.lo, 64u >> r.args.tsh);
    }
    CHECK(next == total, "the ranges end at slot %llu of %llu", next, total);
    CHECK(most == p.most && p.lds == (size_t)64 * g.pitch * sizeof(double) && p.lds <= 159 * 1024, "most %llu (%llu), lds %zu", p.most, most, p.lds);
    for (size_t i = 0; i < cover.size(); ++i) CHECK(cover[i] == 1, "slab (%zu, %zu) lies in %u ranges", i / g.z0, i % g.z0, cover[i]);
    for (size_t i = 0; i < p.size() && !fails; ++i) {
        const std::string w = what + " range " + std::to_string(i);
        check_slots(w, p[i]);
        check_grid(w, p[i]);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return std::printf("usage: %s <table>\n", argv[0]), 2;
    std::ifstream in(argv[1]);
    if (!in) return std::printf("cannot read %s\n", argv[1]), 2;
    std::string line;
    int ncases = 0, accepted = 0, brute = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        Case c;
        std::string what, want;
        if (!parse(line, c, want)) return std::printf("malformed line: %s\n", line.c_str()), 2;
        what = inputs(c);
        ++ncases;
        PairPlan p;
        const bool ok = pair_plan(c.shape(), c.W, c.W == 2 ? 4 : 8, c.cap, c.lanes, c.avail != 0, p);
        const std::string got = dump(ok, p);
        if (got != want) {  // (field for field: the first token that differs)
            std::istringstream a(got), b(want);
            std::string ta, tb;
            int k = 0;
            while (a >> ta, b >> tb, ta == tb && !ta.empty()) ta.clear(), tb.clear(), ++k;
            if (fails++ < 20) std::printf("FAIL %s: token %d is '%s', the table has '%s'\n", what.c_str(), k, ta.c_str(), tb.c_str());
            continue;
        }
        if (!ok) continue;
        ++accepted;
        size_t zrows = 1;
        for (int i = 0; i + 1 < c.nd; ++i) zrows *= c.zs[i];
        if (zrows > 100000) continue;
        ++brute;
        check_plan(what, c, p);
    }
    std::printf("%d cases, %d accepted, %d checked by brute force, %d failures\n", ncases, accepted, brute, fails);
    if (fails || ncases < 300 || brute < 200) return 1;
    std::printf("pair_plan ok\n");
    return 0;
}
