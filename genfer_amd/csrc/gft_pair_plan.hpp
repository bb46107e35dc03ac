// The launch plan of the row-pair form of the reference-order product (k_pair_sums + k_pair_collect, gft_conv_staged.hip):
// whether the form applies, the kernels' arguments, the slab ranges a product is cut into under the workspace cap, one or
// two lanes, and per range the phase-1 grid that k_pair_sums decodes its workgroup index with.  The kernel trusts these sums
// completely — a disagreement writes row sums to the wrong slots or past the workspace — so they live here, without HIP,
// where a plain C++ compiler can check them (tests/pair_plan_check.cpp: against the recorded table and by brute force).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define GFT_PAIR_HD __host__ __device__
#else
#define GFT_PAIR_HD
#endif

namespace gft {

struct PairArgs {
    unsigned xU, x0, x1, yU, y0, y1, zU, z0, z1;  // canonical outer extents (rank 2: U = axis 0 = 1; rank 3: U = 1)
    unsigned n2, nx2, n8, nb, nxc;                // row lengths, padded row length, column blocks, x chunks
    unsigned tsh;                                 // lane tile: T1 = 1 << tsh rows along axis 1, T0 = 64 >> tsh along axis 0
    unsigned NW, xch;                             // waves and x rows of a phase-1 workgroup
    unsigned tiles0, tiles1;                      // y tiles along the two lane axes
    unsigned pitch;                               // LDS row pitch in doubles ((lo, hi) interleaved; pitch / 2 odd)
    unsigned long long S0, S1;                    // terms summed over all k0 / all k1
    // Bounded workspace (round 5): a launch covers the output slabs [klo, khi) of the LEADING outer axis only, and its slots
    // start at slot_base.  band 2: the leading axis is U (rank 4) — the x rows' ju is restricted; band 1: it is axis 0 (rank 3),
    // a lane axis — the y tile is the WINDOW d0 = klo - j0 + l0 of T0 = khi - klo rows under one j0 (every lane of it pairs with
    // an output slab of the range), a workgroup's x rows share that j0.  band 0: the whole product (klo = 0).
    unsigned band, klo, khi;
    unsigned long long slot_base;
    // Phase-1 grid: one workgroup per VALID (x rows, y tile) combination, in one dimension (see k_pair_sums): c1tot chunks of
    // x rows over all tiles of axis 1, s0tot (j0, tile of axis 0) combinations (band 1: j0 from at_lo up, one window each)
    unsigned c1tot, s0tot, at_lo;
    unsigned kuf;  // band 1: the slab of U the range lies in (rank 3: 0) — the x rows' ju = kuf - ud for every y slab ud that has one
};
// terms of output index k on one axis: j in [max(0, k + 1 - ny), min(k + 1, nx)), and the number of terms of all k' < k
GFT_PAIR_HD inline unsigned pair_lo(unsigned k, unsigned ny) { return k + 1 > ny ? k + 1 - ny : 0u; }
GFT_PAIR_HD inline unsigned pair_cnt(unsigned k, unsigned nx, unsigned ny) {
    const unsigned lo = pair_lo(k, ny), hi = k + 1 < nx ? k + 1 : nx;
    return hi > lo ? hi - lo : 0u;
}
GFT_PAIR_HD inline unsigned long long pair_pre(unsigned k, unsigned nx, unsigned ny) {  // sum_{i < k} pair_cnt(i) (for x, y <= z: no empty k)
    const unsigned long long kk = k;
    const unsigned long long A = k <= nx ? kk * (kk + 1) / 2 : (unsigned long long)nx * (nx + 1) / 2 + (kk - nx) * nx;  // sum min(i + 1, nx)
    const unsigned long long B = k > ny ? (kk - ny) * (kk - ny + 1) / 2 : 0ull;                                   // sum max(0, i + 1 - ny)
    return A - B;
}

// The product as the planner sees it (ConvArgs' shape fields: extents and strides in elements, `nd` of each).
struct PairShape {
    int nd;
    const unsigned *xs, *ys, *zs;
    const size_t *xstr, *ystr, *zstr;
    bool operands_slack;  // 64 bytes after x's last element are readable
};

// One launch pair (phase 1, phase 2) on one workspace.
struct PairRange {
    unsigned lo, hi, band, ku;  // band 0: the whole product; 2: slabs [lo, hi) of U (rank 4); 1: slabs [lo, hi) of axis 0 inside slab ku of U (rank 3: ku = 0)
    unsigned long long base, slots;  // its row sums: slots [base, base + slots) of the product's
    PairArgs args;                   // what both kernels are launched with
    unsigned nwg, nrows;             // workgroups of k_pair_sums; output rows (workgroups along x of k_pair_collect)
};

struct PairPlan {
    PairRange one;               // a product whose row sums fit the cap is one range: the hot case, kept off the heap
    std::vector<PairRange> cut;  // else its slab ranges, in slot order
    bool use_lanes;              // the ranges alternate between two streams, each with a workspace of its own
    unsigned long long most;     // bytes of the largest range's row sums: what a workspace must hold
    size_t lds;                  // dynamic LDS of k_pair_sums
    size_t size() const { return cut.empty() ? 1 : cut.size(); }
    const PairRange& operator[](size_t i) const { return cut.empty() ? one : cut[i]; }
    PairRange& operator[](size_t i) { return cut.empty() ? one : cut[i]; }
};

// Operands and result contiguous, no empty axis, x and y inside z: the rows (last axis) of each.
inline bool pair_rows(const PairShape& s, size_t& xrows, size_t& yrows, size_t& zrows) {
    size_t xn = 1, yn = 1, zn = 1;
    for (int ax = s.nd - 1; ax >= 0; --ax) {
        if (s.xstr[ax] != xn || s.ystr[ax] != yn || s.zstr[ax] != zn) return false;
        if (s.xs[ax] == 0 || s.ys[ax] == 0 || s.xs[ax] > s.zs[ax] || s.ys[ax] > s.zs[ax]) return false;
        xn *= s.xs[ax];
        yn *= s.ys[ax];
        zn *= s.zs[ax];
    }
    xrows = xn / s.xs[s.nd - 1];
    yrows = yn / s.ys[s.nd - 1];
    zrows = zn / s.zs[s.nd - 1];
    return true;
}

// The arguments every range of the product shares.
inline PairArgs pair_args(const PairShape& s, int W, size_t xrows) {
    PairArgs g;
    std::memset(&g, 0, sizeof(g));
    g.xU = g.x0 = g.x1 = g.yU = g.y0 = g.y1 = g.zU = g.z0 = g.z1 = 1;
    const int no = s.nd - 1;
    if (no == 1) {
        g.x1 = s.xs[0]; g.y1 = s.ys[0]; g.z1 = s.zs[0];
    } else if (no == 2) {
        g.x0 = s.xs[0]; g.y0 = s.ys[0]; g.z0 = s.zs[0];
        g.x1 = s.xs[1]; g.y1 = s.ys[1]; g.z1 = s.zs[1];
    } else {
        g.xU = s.xs[0]; g.yU = s.ys[0]; g.zU = s.zs[0];
        g.x0 = s.xs[1]; g.y0 = s.ys[1]; g.z0 = s.zs[1];
        g.x1 = s.xs[2]; g.y1 = s.ys[2]; g.z1 = s.zs[2];
    }
    g.n2 = s.zs[no];
    g.nx2 = s.xs[no];
    g.n8 = (g.n2 + 7) / 8 * 8;
    g.nb = g.n8 / 8;
    g.nxc = (g.nx2 + 7) / 8;
    // lane tile: the shape with the fewest lanes outside y's rows (ties: the squarest)
    double best = -1.0;
    for (unsigned tsh = 0; tsh <= 6; ++tsh) {
        const unsigned T1 = 1u << tsh, T0 = 64u >> tsh;
        const double e = (double)g.y0 / ((g.y0 + T0 - 1) / T0 * T0) * (double)g.y1 / ((g.y1 + T1 - 1) / T1 * T1);
        const double pref = e - 1e-6 * (tsh > 3 ? tsh - 3 : 3 - tsh);
        if (pref > best) {
            best = pref;
            g.tsh = tsh;
        }
    }
    const unsigned T1 = 1u << g.tsh, T0 = 64u >> g.tsh;
    g.tiles0 = (std::min(g.y0, g.z0) + T0 - 1) / T0;  // (y rows at or beyond z's extent pair with nothing)
    g.tiles1 = (std::min(g.y1, g.z1) + T1 - 1) / T1;
    g.pitch = W * g.n8 + 2;
    // 16 waves per CU (the kernel holds <= 128 VGPRs): two workgroups of 8 where two tiles fit the LDS, else one of 16
    g.NW = (size_t)64 * g.pitch * sizeof(double) * 2 + 1024 <= 160 * 1024 ? 8u : 16u;
    constexpr unsigned PAIR_XCH = 8;  // x rows per phase-1 workgroup (sweep in profiles/r04/interval_pairs_sweep.txt: 4 .. 12 equal, 32 loses 10 % to the last round of workgroups)
    g.xch = PAIR_XCH;
    // (small products: fewer x rows per workgroup until there are ~1000 workgroups — half of the (tile, chunk) grid is
    // outside the triangle)
    while (g.xch > 1 && (unsigned long long)g.yU * g.tiles0 * g.tiles1 * ((xrows + g.xch - 1) / g.xch) < 2048ull) g.xch /= 2;
    g.S0 = pair_pre(g.z0, g.x0, g.y0);  // terms over all k0 / all k1
    g.S1 = pair_pre(g.z1, g.x1, g.y1);
    return g;
}

// Ranges of 1, 2, 4 or 8 slabs of axis 0 (a lane axis: the range's height is the window's) inside slab ku of U, each within
// range_cap bytes; false: one slab of axis 0 alone exceeds it (not this form's product).
inline bool pair_cut_axis0(const PairArgs& g, unsigned ku, unsigned long long row_bytes, size_t range_cap, std::vector<PairRange>& out) {
    const unsigned long long cU = pair_cnt(ku, g.xU, g.yU), ubase = pair_pre(ku, g.xU, g.yU) * g.S0 * g.S1;
    auto sl = [&](unsigned lo, unsigned hi) { return cU * (pair_pre(hi, g.x0, g.y0) - pair_pre(lo, g.x0, g.y0)) * g.S1; };
    for (unsigned lo = 0; lo < g.z0;) {
        unsigned h = 8;
        while (h >= 1 && !(lo + h <= g.z0 && sl(lo, lo + h) * row_bytes <= range_cap)) h /= 2;
        if (h == 0) return false;
        PairRange r;
        r.lo = lo, r.hi = lo + h, r.band = 1, r.ku = ku;
        r.base = ubase + cU * pair_pre(lo, g.x0, g.y0) * g.S1;
        r.slots = sl(lo, lo + h);
        out.push_back(r);
        lo += h;
    }
    return true;
}

// The product in slab ranges of its leading outer axis, each within range_cap bytes.  Rank 3: ranges of axis 0.  Rank 4: ranges
// of slabs of U where a slab fits, ranges of axis 0 INSIDE a slab of U where it does not (32^4: the top slab alone is 4.6 GB).
inline bool pair_cut(const PairArgs& g, int no, unsigned long long row_bytes, size_t range_cap, std::vector<PairRange>& out) {
    out.clear();
    if (no == 2) return pair_cut_axis0(g, 0, row_bytes, range_cap, out) && out.size() <= 4096;
    auto sl = [&](unsigned lo, unsigned hi) { return (pair_pre(hi, g.xU, g.yU) - pair_pre(lo, g.xU, g.yU)) * g.S0 * g.S1; };
    for (unsigned lo = 0; lo < g.zU;) {
        unsigned h = 0;
        while (lo + h < g.zU && sl(lo, lo + h + 1) * row_bytes <= range_cap) ++h;
        if (h) {
            PairRange r;
            r.lo = lo, r.hi = lo + h, r.band = 2, r.ku = 0;
            r.base = pair_pre(lo, g.xU, g.yU) * g.S0 * g.S1;
            r.slots = sl(lo, lo + h);
            out.push_back(r);
            lo += h;
        } else {
            if (!pair_cut_axis0(g, lo, row_bytes, range_cap, out)) return false;
            lo += 1;
        }
    }
    return out.size() <= 4096;
}

// (x rows sharing (ju, j0)) x (tiles over U and axis 0) of a range whose lane tile is the product's (bands 0 and 2)
inline unsigned long long pair_combos(const PairRange& r, PairArgs& q) {
    const unsigned T0 = 64u >> q.tsh;
    unsigned long long s0 = 0, sU = 0;
    for (unsigned at = 0; at < q.tiles0; ++at) s0 += std::min(q.z0 - T0 * at, q.x0);
    for (unsigned ud = 0; ud < std::min(q.yU, q.zU); ++ud) {
        unsigned nU = std::min(q.zU - ud, q.xU);
        if (r.band == 2) {
            const unsigned ju_lo = r.lo > ud ? r.lo - ud : 0u, hi = r.hi > ud ? std::min(r.hi - ud, nU) : 0u;
            nU = hi > ju_lo ? hi - ju_lo : 0u;
        }
        sU += nU;
    }
    q.s0tot = (unsigned)s0;
    return s0 * sU;
}

// The range's arguments and grids from the product's; false: a grid beyond what a launch takes.
inline bool pair_range_finish(const PairArgs& g, size_t zrows, PairRange& r) {
    PairArgs& q = r.args;
    q = g;
    q.band = r.band;
    q.kuf = r.ku;
    q.klo = r.lo;
    q.khi = r.hi;
    q.slot_base = r.base;
    unsigned long long nrows = zrows, combos = 0;
    if (r.band == 1) {  // window tiles: T0 = the range's height, one per j0; a workgroup's x rows share j0
        const unsigned h = r.hi - r.lo;
        unsigned tsh = 6;
        while ((64u >> tsh) < h) --tsh;
        q.tsh = tsh;
        const unsigned T1 = 1u << tsh;
        q.tiles1 = (std::min(q.y1, q.z1) + T1 - 1) / T1;
        q.tiles0 = std::min(q.x0, r.hi);                   // j0 <= k0 < khi
        q.at_lo = r.lo + 1 > q.y0 ? r.lo + 1 - q.y0 : 0u;  // (a compact y: the window of a lower j0 lies above y's last row)
        const unsigned ud_lo = r.ku + 1 > q.xU ? r.ku + 1 - q.xU : 0u, ud_hi = std::min(q.yU - 1, r.ku);  // y slabs ud with an x slab ju = ku - ud
        combos = q.tiles0 > q.at_lo && ud_hi >= ud_lo ? (unsigned long long)(q.tiles0 - q.at_lo) * (ud_hi - ud_lo + 1) : 0u;
        nrows = (unsigned long long)h * q.z1;
    } else {
        combos = pair_combos(r, q);
        if (r.band == 2) nrows = (unsigned long long)(r.hi - r.lo) * q.z0 * q.z1;
    }
    const unsigned T1 = 1u << q.tsh;
    unsigned long long c1 = 0;
    for (unsigned bt = 0; bt < q.tiles1; ++bt) c1 += (std::min(q.z1 - T1 * bt, q.x1) + q.xch - 1) / q.xch;
    q.c1tot = (unsigned)c1;
    const unsigned long long nwg = combos * q.c1tot;
    if (nwg == 0 || nwg > 0x7fffffffull || nrows > 0x7fffffffull) return false;
    r.nwg = (unsigned)nwg;
    r.nrows = (unsigned)nrows;
    return true;
}

// The plan of the plain full product x * y -> z of elements of W doubles (1 = f64, 2 = interval; CW: the kernel's column block)
// under a workspace cap of `cap` bytes.  lanes_mode: 0 never two lanes, 1 always (where lanes_available), negative: when half
// the cap leaves the ranges as they are.  false: not this form's product, nothing to launch.  Whether the product is WORTH
// this form (its size against the callers' thresholds) is the caller's question.
inline bool pair_plan(const PairShape& s, int W, int CW, size_t cap, int lanes_mode, bool lanes_available, PairPlan& p) {
    p.cut.clear();
    p.use_lanes = false;
    const int nd = s.nd;
    if (nd < 2 || nd > 4) return false;
    const unsigned n2 = s.zs[nd - 1], nx2 = s.xs[nd - 1];
    // (rows beyond 128 intervals / 256 doubles: the tile's 64 y rows no longer fit the LDS)
    if (s.ys[nd - 1] != n2 || n2 < 8 || n2 > (W == 2 ? 128u : 256u) || nx2 == 0) return false;
    size_t xrows, yrows, zrows;
    if (!pair_rows(s, xrows, yrows, zrows)) return false;
    for (int ax = 0; ax + 1 < nd; ++ax)
        if (s.zs[ax] > s.xs[ax] + s.ys[ax] - 1) return false;  // (an output row without terms: the slot prefix sums assume none)
    if (!s.operands_slack && nx2 % CW != 0) return false;  // (the scalar loads of x's last chunk read to the chunk's end: a caller's raw buffer may end with the row)
    const PairArgs g = pair_args(s, W, xrows);
    const unsigned long long slots = pair_pre(g.zU, g.xU, g.yU) * g.S0 * g.S1;
    const unsigned long long row_bytes = (unsigned long long)n2 * W * sizeof(double);
    if (slots == 0 || zrows > 0x7fffffffull) return false;
    // ---- one launch pair for the whole product, or slab ranges of the leading outer axis that fit the cap
    if (slots * row_bytes <= cap) {
        p.one.lo = p.one.hi = p.one.band = p.one.ku = 0;
        p.one.base = 0;
        p.one.slots = slots;
    } else if (nd >= 3) {
        // Two lanes need two workspaces, so each gets half the cap: taken when that does not make the ranges thinner — then
        // one lane's phase 2 (a few hundred one-wave rows: latency, not bandwidth) runs under the other's phase 1.
        // MI355X, positive / mixed-sign: 56^3 2.88 / 5.92 -> 2.55 / 5.05 ms, 64^3 5.31 / 11.5 -> 4.92 / 10.2, 72^3 9.40 / 21.0 -> 8.84 / 20.5;
        // from 80^3 on half the cap halves the window's height and the lanes lose (88^3 29.9 -> 30.4, 96^3 49.8 -> 54.0): off there.
        const bool forced = lanes_mode == 1 && lanes_available;
        if (!pair_cut(g, nd - 1, row_bytes, forced ? cap / 2 : cap, p.cut)) return false;
        p.use_lanes = forced;
        if (lanes_mode < 0 && lanes_available && p.cut.size() >= 2) {
            std::vector<PairRange> half;
            if (pair_cut(g, nd - 1, row_bytes, cap / 2, half) && half.size() == p.cut.size()) {
                p.cut.swap(half);
                p.use_lanes = true;
            }
        }
    } else
        return false;
    if (p.size() < 2) p.use_lanes = false;
    p.most = 0;
    p.lds = (size_t)64 * g.pitch * sizeof(double);
    // (every range BEFORE the first launch: a false return promises that nothing was launched)
    for (size_t i = 0; i < p.size(); ++i) {
        p.most = std::max(p.most, p[i].slots * row_bytes);
        if (!pair_range_finish(g, zrows, p[i])) return false;
    }
    return true;
}

}  // namespace gft
