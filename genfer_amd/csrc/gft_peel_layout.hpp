// The workspace of one peeled tiled product (conv_tiled_peel, gft_conv_tiled.hip): byte offsets of everything its three
// launches — the aligned main part M and the leftover products L0, L1 — keep there, as a plain function of the plans' slot
// counts and the shape:
//   [ticket counters][slabs M][slabs L0][slabs L1][packed x][packed y][L0 window][L1 scalar + slack][L1 window]
// Each launch has partial slabs of its OWN: the leftover launches' main kernels may then run beside M (two lanes), and
// nothing one of them writes is a byte another reads or writes before the join.  It is ONE layout whether or not a call
// forks, claims or packs, so a size query and the launches that follow it agree.  The kernels trust these sums completely —
// a disagreement puts one launch's slabs over another's operands — so they live here, without HIP, where a plain C++
// compiler can check them (tests/peel_layout_check.cpp: disjoint, aligned, inside `need`, monotone).
#pragma once
#include <cstddef>

namespace gft {

constexpr size_t PEEL_ALIGN = 256;        // every region starts on a multiple of it
constexpr size_t PEEL_CLAIM_BYTES = 256;  // ticket counters: eight words per launch, three launches (and spare)
constexpr size_t PEEL_SLAB_DOUBLES = 512; // one partial slab holds 64 lanes x 8 outputs per 8-wide output block

struct PeelLayout {
    // byte offsets; a region's length is what the sizes below say, its end at most the next region's offset
    size_t o_claim, o_slab[3], o_xp, o_yp, o_w0, o_s1, o_w1;
    size_t b_claim, b_slab[3], b_xp, b_yp, b_w0, b_s1, b_w1;  // bytes in use (not rounded)
    size_t need;                                              // bytes of the whole workspace
};

inline size_t peel_align(size_t v) { return (v + PEEL_ALIGN - 1) / PEEL_ALIGN * PEEL_ALIGN; }

// slots[i]: partial slabs of launch i (M, L0, L1), each nb blocks of PEEL_SLAB_DOUBLES doubles; claims: any of the launches
// takes tickets; the remaining arguments are lengths in doubles (slack included).
inline PeelLayout peel_layout(const size_t (&slots)[3], size_t nb, bool claims, size_t xp_doubles, size_t yp_doubles, size_t w0_doubles,
                              size_t s1_doubles, size_t w1_doubles) {
    PeelLayout L;
    size_t at = 0;
    auto put = [&at](size_t bytes, size_t& off, size_t& len) {
        off = at;
        len = bytes;
        at += peel_align(bytes);
    };
    put(claims ? PEEL_CLAIM_BYTES : 0, L.o_claim, L.b_claim);
    for (int i = 0; i < 3; ++i) put(slots[i] * nb * PEEL_SLAB_DOUBLES * sizeof(double), L.o_slab[i], L.b_slab[i]);
    put(xp_doubles * sizeof(double), L.o_xp, L.b_xp);
    put(yp_doubles * sizeof(double), L.o_yp, L.b_yp);
    put(w0_doubles * sizeof(double), L.o_w0, L.b_w0);
    put(s1_doubles * sizeof(double), L.o_s1, L.b_s1);
    put(w1_doubles * sizeof(double), L.o_w1, L.b_w1);
    L.need = at + PEEL_ALIGN;
    return L;
}

// The same from the product's shape: full n0 x n1 operands of padded inner length n8 = 8 nb (n0, n1 multiples of 8).
//   packed x: its rows and one chunk of slack; packed y: its rows; L0 window: the gathered slabs of x, 7 per tile of axis 0;
//   L1 scalar: y's first seven rows of every slab, and one chunk of slack; L1 window: 7 gathered rows per tile of axis 1.
inline PeelLayout peel_layout_for(const size_t (&slots)[3], size_t n0, size_t n1, size_t n8, bool claims) {
    const size_t rows = n0 * n1;
    return peel_layout(slots, n8 / 8, claims, rows * n8 + 8, rows * n8, 7 * (n0 / 8) * n1 * n8, 7 * n0 * n8 + 8, 7 * (n1 / 8) * n0 * n8);
}

}  // namespace gft
