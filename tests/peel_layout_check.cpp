// gft_peel_layout.hpp, the workspace of a peeled tiled product, checked on the CPU: over a grid of shapes and slot counts
// every region is 256-byte aligned, the regions are pairwise disjoint and lie inside `need`, and `need` never falls when
// a launch gets more partial slabs.  (The launches' kernels take these offsets as they are: two regions that overlap
// would put one launch's partial slabs over another's, or over the operands that a launch beside it is still reading.)
#include <cstdio>
#include <vector>

#include "gft_peel_layout.hpp"

using gft::PeelLayout;

struct Region {
    const char* name;
    size_t off, len;
};

static int failures = 0;
static void fail(const char* what, const char* a, const char* b, const size_t (&slots)[3], size_t n0, size_t n1, size_t n8, bool claims) {
    if (++failures <= 20)
        std::printf("FAIL %s %s %s: slots %zu %zu %zu, n0 %zu n1 %zu n8 %zu claims %d\n", what, a, b, slots[0], slots[1], slots[2], n0, n1, n8,
                    (int)claims);
}

static std::vector<Region> regions(const PeelLayout& L) {
    return {{"claim", L.o_claim, L.b_claim},      {"slabs M", L.o_slab[0], L.b_slab[0]}, {"slabs L0", L.o_slab[1], L.b_slab[1]},
            {"slabs L1", L.o_slab[2], L.b_slab[2]}, {"packed x", L.o_xp, L.b_xp},          {"packed y", L.o_yp, L.b_yp},
            {"L0 window", L.o_w0, L.b_w0},        {"L1 scalar", L.o_s1, L.b_s1},         {"L1 window", L.o_w1, L.b_w1}};
}

int main() {
    const size_t extents[] = {16, 24, 64, 128}, inner[] = {8, 20, 64, 128};
    // from one slab up to a few thousand; M's and the leftovers' chosen independently (leftovers larger than M included)
    const size_t counts[] = {1, 2, 3, 7, 64, 511, 1024, 4097};
    unsigned long long points = 0;
    for (size_t n0 : extents)
        for (size_t n1 : extents)
            for (size_t nI : inner)
                for (int claims = 0; claims < 2; ++claims)
                    for (size_t sm : counts)
                        for (size_t s0 : counts)
                            for (size_t s1 : counts) {
                                const size_t n8 = (nI + 7) / 8 * 8, nb = n8 / 8;
                                const size_t slots[3] = {sm, s0, s1};
                                const PeelLayout L = gft::peel_layout_for(slots, n0, n1, n8, claims != 0);
                                const std::vector<Region> R = regions(L);
                                ++points;
                                // the sizes are the ones the kernels use
                                for (int i = 0; i < 3; ++i)
                                    if (L.b_slab[i] != slots[i] * nb * 512 * sizeof(double)) fail("slab bytes", R[1 + i].name, "", slots, n0, n1, n8, claims);
                                if (L.b_claim != (claims ? 256u : 0u)) fail("claim bytes", "", "", slots, n0, n1, n8, claims);
                                if (L.b_xp != (n0 * n1 * n8 + 8) * sizeof(double) || L.b_yp != n0 * n1 * n8 * sizeof(double))
                                    fail("operand bytes", "", "", slots, n0, n1, n8, claims);
                                if (L.b_w0 != 7 * (n0 / 8) * n1 * n8 * sizeof(double) || L.b_s1 != (7 * n0 * n8 + 8) * sizeof(double) ||
                                    L.b_w1 != 7 * (n1 / 8) * n0 * n8 * sizeof(double))
                                    fail("gather bytes", "", "", slots, n0, n1, n8, claims);
                                for (size_t i = 0; i < R.size(); ++i) {
                                    if (R[i].off % 256) fail("alignment", R[i].name, "", slots, n0, n1, n8, claims);
                                    if (R[i].off + R[i].len > L.need) fail("outside need", R[i].name, "", slots, n0, n1, n8, claims);
                                    for (size_t j = i + 1; j < R.size(); ++j) {
                                        const bool apart = R[i].off + R[i].len <= R[j].off || R[j].off + R[j].len <= R[i].off;
                                        if (!apart) fail("overlap", R[i].name, R[j].name, slots, n0, n1, n8, claims);
                                    }
                                }
                                // monotone: one more slab for any launch never needs less
                                for (int i = 0; i < 3; ++i) {
                                    size_t more[3] = {sm, s0, s1};
                                    more[i] += 1;
                                    if (gft::peel_layout_for(more, n0, n1, n8, claims != 0).need < L.need) fail("not monotone", R[1 + i].name, "", slots, n0, n1, n8, claims);
                                }
                            }
    // monotone along the whole count list too (not only by one slab)
    for (int i = 0; i < 3; ++i) {
        size_t prev = 0;
        for (size_t c : counts) {
            size_t slots[3] = {5, 5, 5};
            slots[i] = c;
            const size_t need = gft::peel_layout_for(slots, 128, 128, 128, true).need;
            if (need < prev) fail("not monotone along the list", "", "", slots, 128, 128, 128, true);
            prev = need;
        }
    }
    if (failures) {
        std::printf("%d failures in %llu grid points\n", failures, points);
        return 1;
    }
    std::printf("%llu grid points\npeel_layout ok\n", points);
    return 0;
}
