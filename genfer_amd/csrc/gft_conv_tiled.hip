// LDS-tiled f64 truncated N-d convolution for gfx950 (the hot loop of TaylorPoly * TaylorPoly,
// src/multivariate_taylor.rs:971-1012) — compute-bound on FP64 FMA, so the design goal is to keep
// the 4 SIMDs of every CU issuing v_fma_f64 with both operands already on-chip:
//
//   canonical problem   z[u][k0][k1][k2] = sum_j x[ju][j0][j1][j2] * y[u-ju][k0-j0][k1-j1][k2-j2]
//                       (rank 3: U = 1; rank 4: U = leading axis)
//   lanes               the 64 lanes of a wave own a T0 x T1 tile of (k0,k1) output ROWS (8x8 by default; 4x16, 2x32 or
//                       1x64 when k0 is short or absent: rank 2, piece-split products); each lane keeps R = 8
//                       consecutive k2 outputs of its row in registers (two such blocks per wave, c and nb-1-c, so
//                       every wave of the workgroup has the same trip count although the index space is triangular)
//   x operand           wave-uniform: x[J][j2..j2+7] comes from scalar loads (constant address space =>
//                       s_load_dwordx16) into SGPRs and is the SGPR source of v_fma_f64 — zero VGPR/LDS
//                       traffic for one of the two operands
//   y operand           a T0 x T1 window of y rows lives in LDS, row slot r at offset r*P1 doubles with P1/2 odd
//                       (conflict-free ds_read_b128 per 16-lane group); each lane slides an 8-wide register window
//                       along its row: 8 new doubles from LDS per 64 FMAs
//   window motion       the step space is walked row by row (a run of j1 steps under one (ju, j0)): stepping j1
//                       replaces one of the T1 ring slots (T0 rows, prefetched global->VGPR during the step, written
//                       to LDS after it); a new row starts with a full window load
//   triangular waste    none along k2 (the diagonal 8x8 chunk is a 36-FMA triangle); (n+8)/(n+1) per
//                       lane axis from masked lanes in diagonal tiles — unless the product is PEELED (rank 3,
//                       full extents, 8x8 lane tile): the main launch then stops every tile's step range at the
//                       tile's first row (TiledArgs::cut, no masked lane left) and the 28-pair leftover triangle
//                       of every tile runs as two small rank-4 products whose batch axis is the tile index
//                       (conv_tiled_peel below)
//   load balance        stream-K: the linearised (tile, ju, j0, j1) step space is cut into equal
//                       contiguous ranges, 1, 2, 4 or 8 per resident workgroup slot (as many as leave a
//                       range >= ~190 steps; fewer for small products, cut_ranges below).  Tiles covered by a
//                       single range are written straight to z; split tiles go through partial slabs
//                       in a workspace and a fixed-order reduce kernel => deterministic results.
//   persistent launch   a plan with more ranges than the device has resident workgroup slots is launched with one
//                       workgroup per slot; each CLAIMS ranges (a ticket from one of eight XCD-local queues, the other
//                       queues once its own is empty) until none is left, and the ranges taper along every queue: large
//                       ones first, small ones last (claim_range, cut_ranges).  The cuts depend on the shape
//                       and the slot count only, never on who runs a range: results do not depend on the schedule.
//
// Numerics: explicit fma (one rounding per MAC) and a different summation order than the
// reference => 1e-10 relative parity, not bit-exact (the reference-order kernels — the LDS-staged and row-pair
// forms in gft_conv_staged.hip, k_conv_naive in gft_kernels.hip — are the bit-exact path).  Zero padding times
// inf / NaN would create NaNs the reference does not produce: k_prep_operands takes the non-finite verdict on the
// device while it packs (a stamp in the guard word), the tiled kernels then leave z alone and the caller's guarded
// reference-order launch computes it; operands read in place have no padding and need no verdict (operand_layout).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "gft_kernels.hpp"
#include "gft_peel_layout.hpp"

namespace gft {

namespace {

struct TileSeg {
    unsigned u, a, b;                // tile coordinates
    unsigned step_begin, step_end;   // range in the tile's linearised (ju, j0, j1) space
    int dest;                        // -1: write z directly; >= 0: workspace slot
};

struct RedTile {
    unsigned u, a, b;
    unsigned first, count;           // pieces: red_slots[first .. first+count)
    unsigned slot0;                  // red_slots == null: the pieces are the workspace slots slot0 .. slot0 + count - 1
};

struct TiledArgs {
    unsigned xU, x0, x1, xI;
    unsigned yU, y0, y1, yI;
    unsigned zU, z0, z1, zI;
    unsigned nx8, ny8;               // padded inner lengths of the packed operands
    unsigned nxc, nyc, nb;           // chunk counts (nx8/8, ny8/8) and number of 8-wide output blocks
    unsigned P1;                     // LDS row pitch in doubles
    unsigned tsh;                    // lane tile: T1 = 1 << tsh lanes along k1, T0 = 64 >> tsh along k0 (8x8 ... 1x64)
    unsigned slab_axis;              // the slab range applies to: 0 = u, 1 = k0, 2 = k1
    unsigned slab_lo, slab_hi;
    int accumulate;
    unsigned xcd_remap;              // 1: remap blockIdx so that each XCD owns a contiguous chunk of ranges
    unsigned cut;                    // bit 0 / 1: the step range of a tile on lane axis 0 / 1 ends at the tile's first row
                                     // (j <= T a instead of j <= T a + T - 1): the aligned part of a peeled product
    unsigned lim1;                   // peel instantiation: lane k1 takes window rows d1 <= 8 (k1 / 8) only
    size_t zsU, zs0, zs1, zoff;      // output strides of (u, k0, k1) and base offset, in doubles (dense unless peeled;
                                     // read by the peel instantiation and by k_conv_reduce)
    const double* xp;
    const double* yp;
    double* z;
    double* ws;
    const TileSeg* segs;
    const unsigned* wg_begin;        // segments of workgroup w: [wg_begin[w], wg_begin[w+1])
    const RedTile* red;
    const unsigned* red_slots;
    const unsigned* guard;           // non-finite verdict word: main/reduce kernels do nothing if *guard == guard_epoch
    unsigned guard_epoch;
    unsigned* claim;                 // persistent launch: the ticket counter of each queue (zero at launch); null: workgroup
                                     // w runs range w (or its XCD-contiguous image, xcd_remap) on the VAR | 256 instantiation
    unsigned n_ranges, n_queues;     // claim: queue q (of 1 or 8) holds the ranges [q, q + 1) * n_ranges / n_queues
#ifdef GFT_TILED_DIAG
    unsigned long long* stamps;      // timeline (GFT_TILED_STAMPS): per range its start and end in s_memrealtime ticks and the
                                     // XCD that ran it (blockIdx & 7); no output is computed from it
#endif
    unsigned char blk1[8], blk2[8];  // output blocks (8 consecutive k2) owned by wave w; 0xff = none
};

// x rows are read through the constant address space: the address is wave-uniform and x is never
// written by this kernel, so hipcc emits s_load_dwordx16 into SGPRs (scalar cache path) instead of
// 64-lane broadcast vector loads that would occupy the texture-address unit.
typedef const double __attribute__((address_space(4))) * cptr_t;

#ifndef GFT_TILED_DEFAULT_VARIANT
#define GFT_TILED_DEFAULT_VARIANT 7
#endif
#ifndef GFT_TILED_PEEL_DEFAULT
#define GFT_TILED_PEEL_DEFAULT -1  // "tiled_peel": -1 auto (by size), 0 never, 1 wherever the structure allows
#endif
#ifndef GFT_TILED_PEEL_LANES_DEFAULT
#define GFT_TILED_PEEL_LANES_DEFAULT -1  // "tiled_peel_lanes": -1 where both leftover launches are persistent, 0 never, 1 wherever a product peels
#endif
// auto mode peels products whose two lane axes are at least PEEL_MIN_EXTENT long and whose inner axis at least
// PEEL_MIN_INNER: the range the sweep covers (profiles/r07/tiled_peel_sweep.txt); a short inner axis leaves the same fixed
// cost (one pack, two more main launches, two more reduces) against a fraction of the work
constexpr unsigned PEEL_MIN_EXTENT = 112, PEEL_MIN_INNER = 64;
// VAR bits: 1 = software-pipelined fast path for full inner extents; 128 = peel instantiation (per-lane row limit on
// axis 1 and strided output, for the leftover products of a peeled product); diagnostics (wrong results, timing
// only, built with -DGFT_TILED_DIAG): 16 = no LDS reads in the chunk loop, 32 = no scalar x loads,
// 64 = no window maintenance / barriers.  256 = one range per workgroup, the static launch of a plan whose ranges all fit
// the device's slots at once (small products): the same kernel without the claiming loop, so that such a launch runs the
// code it ran before there was one; without the bit the workgroups claim (TiledArgs::claim is then never null).

__device__ inline void loadx(double (&dst)[8], cptr_t p) {  // wave-uniform: 8 doubles -> 16 SGPRs
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = p[i];
}

__device__ inline void load8(double (&dst)[8], const double* p) {
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = p[i];
}

// 16-byte aligned window chunk: four ds_read_b128 (4 LDS cycles each) instead of four ds_read2_b64 (8 each)
__device__ inline void load8_b128(double (&dst)[8], const double* p) {
    const double2* q = reinterpret_cast<const double2*>(__builtin_assume_aligned(p, 16));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double2 v = q[i];
        dst[2 * i] = v.x;
        dst[2 * i + 1] = v.y;
    }
}

__device__ inline void fma_rows(double (&acc)[8], const double (&xq)[8], const double (&cur)[8],
                                const double (&prev)[8], int s_lo, int s_hi) {
    // acc[r] += x[8q+s] * y[8(c-q) + r - s]; r-s >= 0 -> cur[r-s], else prev[8 + r - s]
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (s < s_lo || s >= s_hi) continue;
        const double xs = xq[s];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const double yv = (r - s >= 0) ? cur[(r - s) & 7] : prev[(8 + r - s) & 7];
            acc[r] = __builtin_fma(xs, yv, acc[r]);
        }
    }
}

__device__ inline void fma_full(double (&acc)[8], const double (&xq)[8], const double (&cur)[8],
                                const double (&prev)[8]) {
    fma_rows(acc, xq, cur, prev, 0, 8);
}

__device__ inline void fma_tri(double (&acc)[8], const double (&xq)[8], const double (&cur)[8]) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const double xs = xq[s];
#pragma unroll
        for (int r = s; r < 8; ++r) acc[r] = __builtin_fma(xs, cur[r - s], acc[r]);
    }
}

// General path: one output block c (8 consecutive k2) of one lane-row for one (x row, y row) pair; handles
// compact operands (fewer x / y chunks than output blocks).
template <int VAR>
__device__ inline void block_mac(double (&acc)[8], unsigned c, cptr_t xr, const double* yrow, unsigned nxc,
                                 unsigned nyc) {
    constexpr bool NO_LDS = (VAR & 16) != 0;
    constexpr bool NO_X = (VAR & 32) != 0;
    unsigned q_lo = c > nyc ? c - nyc : 0;
    unsigned q_hi = c < nxc ? c : nxc;  // full chunks q in [q_lo, q_hi)
    double A[8], B[8], X[8];
    unsigned m0 = c - q_lo;
    if (m0 < nyc) {
        load8(A, yrow + 8 * m0);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) A[i] = 0.0;
    }
    if (NO_LDS) load8(B, yrow);
    if (NO_X) loadx(X, xr);
    unsigned q = q_lo;
    // two chunks per iteration so the sliding window alternates between A and B without moves
    for (; q + 2 <= q_hi; q += 2) {
        if (!NO_LDS) load8(B, yrow + 8 * (c - q - 1));
        if (!NO_X) loadx(X, xr + 8 * q);
        fma_full(acc, X, A, B);
        if (!NO_LDS) load8(A, yrow + 8 * (c - q - 2));
        if (!NO_X) loadx(X, xr + 8 * (q + 1));
        fma_full(acc, X, B, A);
    }
    if (q < q_hi) {
        if (!NO_LDS) load8(B, yrow + 8 * (c - q - 1));
        if (!NO_X) loadx(X, xr + 8 * q);
        fma_full(acc, X, A, B);
        if (c < nxc) {
            if (!NO_X) loadx(X, xr + 8 * c);
            fma_tri(acc, X, B);
        }
    } else if (c < nxc) {
        if (!NO_X) loadx(X, xr + 8 * c);
        fma_tri(acc, X, A);
    }
}

// Fast path (x and y span every chunk the block touches: q_lo = 0, q_hi = c).  The window buffers rotate three ways
// (A, B, C: current, previous, in flight), the x buffers two ways (X0, X1 — 32 SGPRs; a third set pushed the kernel's
// scalar state out of the register file, and every per-step scalar then cost a v_readlane from a spill lane): chunk i
// uses (X_i; cur, prev) and, right after its first FMA row — i.e. after the s_waitcnt that the first use of its own
// operands triggers — requests x[q+i+1] and W[q+i+2] for the following chunks.  Every LDS / scalar-load result is
// therefore >= 56 FMAs (~250 cycles) old when first used, and the window slides without register moves.  The
// scheduling barriers pin this order (hipcc otherwise sinks the loads next to their uses and stalls on them).
// The diagonal triangle (x chunk c against y chunk 0) goes FIRST, on the buffers the pipeline fills last (X1, C), so
// the chunk loop needs no per-remainder epilogues: six phases (the rotation's period), then up to five of them again.
// W[t] = yrow[8(c-t) ..+7]; t = c+1 reads the row's 8-double front padding — loaded but never used.
#define GFT_STEP(XU, CUR, PREV, XN, TX, WN, TW)                 \
    do {                                                        \
        fma_rows(acc, XU, CUR, PREV, 0, 1);                     \
        __builtin_amdgcn_sched_barrier(0);                      \
        if (!NO_X) loadx(XN, xr + 8 * (TX));                    \
        if (!NO_LDS) { if (B128) load8_b128(WN, w0 - 8 * (int)(TW)); else load8(WN, w0 - 8 * (int)(TW)); } \
        __builtin_amdgcn_sched_barrier(0);                      \
        fma_rows(acc, XU, CUR, PREV, 1, 8);                     \
    } while (0)
#define GFT_PH0 GFT_STEP(X0, A, B, X1, q + 1, C, q + 2)
#define GFT_PH1 GFT_STEP(X1, B, C, X0, q + 2, A, q + 3)
#define GFT_PH2 GFT_STEP(X0, C, A, X1, q + 3, B, q + 4)
#define GFT_PH3 GFT_STEP(X1, A, B, X0, q + 4, C, q + 5)
#define GFT_PH4 GFT_STEP(X0, B, C, X1, q + 5, A, q + 6)
#define GFT_PH5 GFT_STEP(X1, C, A, X0, q + 6, B, q + 7)
// chunks q .. q_hi-1 with (X0; A, B) holding chunk q's operands
#define GFT_CHUNK_LOOP(Q_HI)                                    \
    do {                                                        \
        for (; q + 6 <= (Q_HI); q += 6) {                       \
            GFT_PH0; GFT_PH1; GFT_PH2; GFT_PH3; GFT_PH4; GFT_PH5; \
        }                                                       \
        const unsigned rem = (Q_HI) - q;                        \
        if (rem >= 1) {                                         \
            GFT_PH0;                                            \
            if (rem >= 2) {                                     \
                GFT_PH1;                                        \
                if (rem >= 3) {                                 \
                    GFT_PH2;                                    \
                    if (rem >= 4) {                             \
                        GFT_PH3;                                \
                        if (rem >= 5) GFT_PH4;                  \
                    }                                           \
                }                                               \
            }                                                   \
        }                                                       \
    } while (0)

template <int VAR>
__device__ inline void block_fast(double (&acc)[8], unsigned c, cptr_t xr, const double* yrow) {
    constexpr bool NO_LDS = (VAR & 16) != 0;
    constexpr bool NO_X = (VAR & 32) != 0;
    constexpr bool B128 = (VAR & 2) != 0;
    const double* w0 = yrow + 8 * c;  // W[t] = w0 - 8t
    double A[8], B[8], C[8], X0[8], X1[8];
    // everything the first two chunks need is requested up front (for c = 0 the pipeline's operands are loaded and never
    // used: x chunk 0, W[0] = the triangle's own window, W[1] = the front padding)
    loadx(X1, xr + 8 * c);
    loadx(X0, xr);
    if (B128) { load8_b128(C, yrow); load8_b128(A, w0); load8_b128(B, w0 - 8); } else { load8(C, yrow); load8(A, w0); load8(B, w0 - 8); }
    __builtin_amdgcn_sched_barrier(0);
    fma_tri(acc, X1, C);
    unsigned q = 0;
    GFT_CHUNK_LOOP(c);
}

// The same pipeline for COMPACT operands (fewer x / y chunks than output blocks: the piece-split products, Horner
// steps with a small substitution): x chunks q in [q_lo, q_hi) with q_lo = max(0, c - nyc), q_hi = min(c, nxc), the
// diagonal triangle only if c < nxc, and the first window is zero when it would lie beyond y's last chunk.
// A separate function (and instantiation, VAR bit 8) so that the full-extent kernel's code is untouched.
template <int VAR>
__device__ inline void block_fast_gen(double (&acc)[8], unsigned c, cptr_t xr, const double* yrow, unsigned nxc,
                                      unsigned nyc) {
    constexpr bool NO_LDS = (VAR & 16) != 0;
    constexpr bool NO_X = (VAR & 32) != 0;
    constexpr bool B128 = (VAR & 2) != 0;
    const unsigned q_lo = c > nyc ? c - nyc : 0, q_hi = c < nxc ? c : nxc;
    const bool tri = c < nxc;
    if (q_hi <= q_lo && !tri) return;
    const double* w0 = yrow + 8 * c;  // W[t] = w0 - 8t = y chunk c - t
    double A[8], B[8], C[8], X0[8], X1[8];
    // the scalar (x) loads are unconditional, on clamped chunk indices: a conditionally loaded SGPR array becomes a phi
    // that hipcc parks in VGPRs (16 of them, and the kernel has none to spare)
    loadx(X1, xr + 8 * (tri ? c : 0u));
    loadx(X0, xr + 8 * (q_hi > q_lo ? q_lo : 0u));
    if (B128) load8_b128(C, yrow); else load8(C, yrow);
    if (c - q_lo < nyc) {
        if (B128) load8_b128(A, w0 - 8 * (int)q_lo); else load8(A, w0 - 8 * (int)q_lo);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) A[i] = 0.0;
    }
    if (B128) load8_b128(B, w0 - 8 * (int)(q_lo + 1)); else load8(B, w0 - 8 * (int)(q_lo + 1));
    __builtin_amdgcn_sched_barrier(0);
    if (tri) fma_tri(acc, X1, C);
    unsigned q = q_lo;
    GFT_CHUNK_LOOP(q_hi);
}

struct TileGeom {
    unsigned julo, n_ju, j0lo, n_j0, j1lo, n_j1;
};

__host__ __device__ inline TileGeom tile_geom(const TiledArgs& A, unsigned tsh, unsigned u, unsigned a, unsigned b) {
    TileGeom g;
    const unsigned T0 = 64u >> tsh, T1 = 1u << tsh;
    // uniform axis: ju in [max(0,u+1-yU), min(u+1,xU))
    g.julo = (u + 1 > A.yU) ? (u + 1 - A.yU) : 0;
    unsigned juhi = (u + 1 < A.xU) ? (u + 1) : A.xU;
    g.n_ju = juhi > g.julo ? juhi - g.julo : 0;
    // lane axes: any lane of the tile valid.  k in [T a, min(T a + T - 1, z - 1)]
    unsigned k0max = (T0 * a + T0 - 1 < A.z0 - 1) ? T0 * a + T0 - 1 : A.z0 - 1;
    g.j0lo = (T0 * a + 1 > A.y0) ? (T0 * a + 1 - A.y0) : 0;
    unsigned j0hi = (k0max + 1 < A.x0) ? (k0max + 1) : A.x0;
    if ((A.cut & 1u) && T0 * a + 1 < j0hi) j0hi = T0 * a + 1;
    g.n_j0 = j0hi > g.j0lo ? j0hi - g.j0lo : 0;
    unsigned k1max = (T1 * b + T1 - 1 < A.z1 - 1) ? T1 * b + T1 - 1 : A.z1 - 1;
    g.j1lo = (T1 * b + 1 > A.y1) ? (T1 * b + 1 - A.y1) : 0;
    unsigned j1hi = (k1max + 1 < A.x1) ? (k1max + 1) : A.x1;
    if ((A.cut & 2u) && T1 * b + 1 < j1hi) j1hi = T1 * b + 1;
    g.n_j1 = j1hi > g.j1lo ? j1hi - g.j1lo : 0;
    return g;
}

constexpr unsigned YPAD = 8;  // front padding of every LDS row (doubles)

// Persistent launch: the next range of this workgroup, or ~0u when every queue is empty.  Called by ONE thread.  A queue
// is a contiguous run of ranges and a ticket counter; workgroup w serves queue w & 7 first — workgroups are dealt
// round-robin over the 8 XCDs, so that is the XCD-contiguous eighth xcd_remap gives the static launch (neighbouring ranges
// share y windows in one L2) — and once a queue has run out it moves on, for good, to the next one in the fixed
// rotation (`rot` queues are behind it).  The atomic is relaxed and device-scope and nothing is fenced: the plan tables
// are read-only and no workgroup reads what another one wrote (a device-scope release / acquire pair costs a write-back
// and an invalidate of the XCD's L2 here, see the note below).  A workgroup overshoots every counter at most once.
__device__ inline unsigned claim_range(const TiledArgs& A, unsigned& rot) {
    const unsigned nq = A.n_queues, per_q = A.n_ranges / nq, home = blockIdx.x & (nq - 1u);
    while (rot < nq) {
        const unsigned q = (home + rot) & (nq - 1u);
        const unsigned t = __hip_atomic_fetch_add(A.claim + q, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t < per_q) return q * per_q + t;
        ++rot;
    }
    return ~0u;
}

// (Round 4 tried the reduction of split tiles INSIDE this kernel once more — a two-level tree of last arrivers: the workgroup
// that stores a piece arrives at its group of 8 consecutive pieces, a group's last arriver sums the group in slab order
// and arrives at the tile, whose last arriver sums the group sums and writes z; deterministic, nobody waits.  Correct, and
// slower at every size: 32^3 48.7 -> 48.4 us, 64^3 447 -> 521 us, 378^2 310 -> 443 us.  Every arrival needs a device-scope
// release + acquire around its counter, which on this part is a write-back and an invalidate of the XCD's whole L2 —
// paid by a thousand workgroups while their neighbours are still streaming y windows through that L2 — and the call kept
// 116 bytes of scratch in the kernel.)

template <int NW, int VAR, int TSH>
__global__ void __launch_bounds__(NW * 64, 4)  // 4 waves per SIMD = 16 waves per CU => <= 128 VGPRs
k_conv_tiled(TiledArgs A) {
    constexpr bool FAST = (VAR & 1) != 0;
    constexpr bool NO_WINDOW = (VAR & 64) != 0;
    constexpr bool PEEL = (VAR & 128) != 0;
    extern __shared__ double lds[];
    // an operand holds inf/NaN: the reference-order kernel (launched next, guarded the other way) owns z
    if (A.guard && *A.guard == A.guard_epoch) return;
    const unsigned tid = threadIdx.x;
    const unsigned lane = tid & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // lane tile T0 x T1 over the (k0, k1) output rows: 8x8 by default (TSH = 3, compile-time); 1x64, 2x32 or 4x16 (TSH = 0:
    // A.tsh at run time) when axis k0 is short or absent — the rank-2 products and the piece-split ones, whose lanes
    // would otherwise sit masked
    const unsigned tsh = TSH ? (unsigned)TSH : A.tsh, T1m = (1u << tsh) - 1u, T0 = 64u >> tsh;
    const unsigned l0 = lane >> tsh, l1 = lane & T1m;
    constexpr unsigned NT = NW * 64;

    const unsigned c1 = A.blk1[wave];
    const unsigned c2 = A.blk2[wave];
    const bool has1 = c1 != 0xffu;
    const bool has2 = c2 != 0xffu;

    const unsigned half_row = A.ny8 >> 1;                  // 16-byte pieces per row
    const unsigned hr_magic = (1u << 24) / half_row + 1u;  // p / half_row == (p * magic) >> 24 for the p < 4096 used here
    const size_t y_row_stride = A.ny8;
    // this thread's piece of a ring-slot refill (one refill = T0 rows of half_row 16-byte pieces; at most one per thread:
    // T0 * ny8 / 2 <= 64 NW because yI <= zI and NW >= nb / 2)
    const unsigned pf_s0 = (tid * hr_magic) >> 24, pf_col = tid - pf_s0 * half_row;
    const bool pf_mine = pf_s0 < T0;
    double* const lds_lane = lds + (size_t)(l0 << tsh) * A.P1 + YPAD;
    double* const lds_pf = lds + (size_t)(pf_s0 << tsh) * A.P1 + YPAD + 2 * pf_col;

    // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs, so give each XCD a CONTIGUOUS eighth of
    // the stream-K ranges — neighbouring ranges sweep overlapping y-row windows and then share one L2.
    unsigned wg = blockIdx.x;
    if (A.xcd_remap) wg = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    // persistent launch: one thread claims, the ticket reaches the others through LDS.  Two words taken in turn, so one
    // barrier per range is enough: word i is rewritten two claims later, behind the barrier of the claim in between.
    // (The words lie behind the window in the dynamic allocation — Plan::lds_bytes — not in a static one: the kernel's
    // dynamic limit is raised to the whole 160 KB, and a static byte on top of that makes the attribute call fail.)
    unsigned* const ticket = reinterpret_cast<unsigned*>(lds + 64 * (size_t)A.P1);
    unsigned& claim_rot = ticket[2];
    constexpr bool claiming = (VAR & 256) == 0;
    if (claiming && tid == 0) claim_rot = 0;
    for (unsigned turn = 0;; turn ^= 1u) {  // (one pass for a static launch; the body keeps the indentation it had without the loop)
    if (claiming) {
        if (tid == 0) {
            unsigned rot = claim_rot;
            ticket[turn] = claim_range(A, rot);
            claim_rot = rot;
        }
        __syncthreads();
        wg = __builtin_amdgcn_readfirstlane(ticket[turn]);
        if (wg == ~0u) break;
    }
#ifdef GFT_TILED_DIAG
    if (A.stamps && tid == 0) {
        A.stamps[3 * (size_t)wg] = __builtin_amdgcn_s_memrealtime();
        A.stamps[3 * (size_t)wg + 2] = blockIdx.x & 7u;
    }
#endif
    const unsigned seg_begin = A.wg_begin[wg], seg_end = A.wg_begin[wg + 1];
    for (unsigned si = seg_begin; si < seg_end; ++si) {
        const TileSeg seg = A.segs[si];
        const unsigned u = seg.u, a = seg.a, b = seg.b;
        const TileGeom g = tile_geom(A, tsh, u, a, b);
        const unsigned k0 = T0 * a + l0, k1 = (b << tsh) + l1;
        bool lane_in = k0 < A.z0 && k1 < A.z1;
        if (A.slab_axis == 1) lane_in = lane_in && k0 >= A.slab_lo && k0 < A.slab_hi;
        else if (A.slab_axis == 2) lane_in = lane_in && k1 >= A.slab_lo && k1 < A.slab_hi;
        // (peel: the window rows this lane may take end at its own tile's first row — the leftover product along axis 1)
        unsigned y1lim = A.y1;
        if (PEEL && A.lim1 && (k1 & ~7u) + 1u < y1lim) y1lim = (k1 & ~7u) + 1u;

        double acc1[8], acc2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc1[i] = acc2[i] = 0.0;

        unsigned tj1 = seg.step_begin % g.n_j1;
        unsigned t = seg.step_begin / g.n_j1;
        unsigned tj0 = t % g.n_j0;
        unsigned ju = g.julo + t / g.n_j0, j0 = g.j0lo + tj0, j1 = g.j1lo + tj1;
        unsigned steps_left = seg.step_end - seg.step_begin;
        const unsigned j1_end = g.j1lo + g.n_j1;

        // The step space is walked row by row: a ROW is a run of j1 steps under one (ju, j0) — it starts with a full
        // window load, and inside it every per-step quantity is a running value (x row pointer, the lane's k1 - j1,
        // the refill piece's source pointer) instead of a function of (ju, j0, j1) recomputed from the plan's scalars.
        while (steps_left) {
            const unsigned row_steps = steps_left < j1_end - j1 ? steps_left : j1_end - j1;
            const double* ybase = A.yp + (size_t)(u - ju) * A.y0 * A.y1 * y_row_stride;
            if (!NO_WINDOW) {
                // (re)load the whole T0 x T1 window of y rows for (ju, j0, j1)
                // (round 4: the <= 8 pieces of a thread are loaded one after the other — each load sits under its range test, a
                // block of its own, and hipcc waits for vmcnt(0) at block boundaries.  Issuing all eight unconditionally first
                // was measured: 16 hoisted per-piece invariants spill, 64^3 410 -> 429 us, 24^4 636 -> 704 us, 128^3 -2 %: the
                // other workgroups of the CU already cover a row start)
                __syncthreads();
                for (unsigned p = tid; p < 64 * half_row; p += NT) {
                    unsigned row = (p * hr_magic) >> 24, col = p - row * half_row;
                    unsigned s0 = row >> tsh, s1 = row & T1m;
                    int R0 = (int)(T0 * a + s0) - (int)j0;
                    int R1 = (int)((b << tsh) + s1) - (int)j1;
                    if (R0 >= 0 && R0 < (int)A.y0 && R1 >= 0 && R1 < (int)A.y1) {
                        const double2 v = *reinterpret_cast<const double2*>(
                            ybase + ((size_t)R0 * A.y1 + (size_t)R1) * y_row_stride + 2 * col);
                        double* d = lds + ((s0 << tsh) + ((unsigned)R1 & T1m)) * A.P1 + YPAD + 2 * col;
                        d[0] = v.x;
                        d[1] = v.y;
                    }
                }
                __syncthreads();
            }
            // running values of the row
            cptr_t xr = (cptr_t)(A.xp + (((size_t)ju * A.x0 + j0) * A.x1 + j1) * A.nx8);  // wave-uniform
            const bool valid0 = lane_in && j0 <= k0 && (k0 - j0) < A.y0;
            int d1 = (int)k1 - (int)j1;               // this lane's y row along axis 1
            int R1n = (int)(b << tsh) - (int)j1 - 1;  // the y row the NEXT step's window gains
            const int pf_R0 = (int)(T0 * a + pf_s0) - (int)j0;
            const bool pf_row = pf_mine && pf_R0 >= 0 && pf_R0 < (int)A.y0;
            const double* pf_src = ybase + ((ptrdiff_t)pf_R0 * (ptrdiff_t)A.y1 + R1n) * (ptrdiff_t)y_row_stride + 2 * pf_col;

            for (unsigned rs = row_steps; rs > 0; --rs) {
                const bool last = rs == 1;  // last step of the row (or of the range): no refill, no barriers
                // prefetch the ring slot that the next j1 step needs: rows (.., R1n) — nothing else is new
                const bool do_pf = !NO_WINDOW && !last && R1n >= 0 && R1n < (int)A.y1;
                double2 pf;
                if (do_pf && pf_row) pf = *reinterpret_cast<const double2*>(pf_src);

                // ---- compute this step -------------------------------------------------------------
                if (valid0 && (unsigned)d1 < (PEEL ? y1lim : A.y1)) {  // j1 <= k1 and k1 - j1 < y1
                    const double* yrow = lds_lane + (size_t)((unsigned)d1 & T1m) * A.P1;
                    if constexpr (FAST && (VAR & 8)) {  // pipelined path for compact operands
                        if (has1) block_fast_gen<VAR>(acc1, c1, xr, yrow, A.nxc, A.nyc);
                        if (has2) block_fast_gen<VAR>(acc2, c2, xr, yrow, A.nxc, A.nyc);
                    } else if constexpr (FAST) {  // host guarantees nxc, nyc >= nb for this instantiation
                        if (has1) block_fast<VAR>(acc1, c1, xr, yrow);
                        if (has2) block_fast<VAR>(acc2, c2, xr, yrow);
                    } else {
                        if (has1) block_mac<VAR>(acc1, c1, xr, yrow, A.nxc, A.nyc);
                        if (has2) block_mac<VAR>(acc2, c2, xr, yrow, A.nxc, A.nyc);
                    }
                }

                // ---- advance within the row ----------------------------------------------------------
                if (!last && !NO_WINDOW) {
                    __syncthreads();  // everyone is done reading the slot being replaced
                    if (do_pf && pf_row) {
                        double* d = lds_pf + (size_t)((unsigned)R1n & T1m) * A.P1;
                        d[0] = pf.x;
                        d[1] = pf.y;
                    }
                    __syncthreads();
                }
                xr += A.nx8;
                d1 -= 1;
                R1n -= 1;
                pf_src -= y_row_stride;
            }
            steps_left -= row_steps;
            // next row
            j1 = g.j1lo;
            if (j0 + 1 < g.j0lo + g.n_j0) j0++;
            else {
                j0 = g.j0lo;
                ju++;
            }
        }

        // ---- write out ---------------------------------------------------------------------------------
        if (seg.dest < 0) {
            if (lane_in) {
                double* zrow = A.z + (((size_t)u * A.z0 + k0) * A.z1 + k1) * A.zI;
                if constexpr (PEEL) zrow = A.z + A.zoff + (size_t)u * A.zsU + (size_t)k0 * A.zs0 + (size_t)k1 * A.zs1;
                if (has1) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        unsigned k2 = 8 * c1 + r;
                        if (k2 < A.zI) zrow[k2] = A.accumulate ? zrow[k2] + acc1[r] : acc1[r];
                    }
                }
                if (has2) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        unsigned k2 = 8 * c2 + r;
                        if (k2 < A.zI) zrow[k2] = A.accumulate ? zrow[k2] + acc2[r] : acc2[r];
                    }
                }
            }
        } else {
            double* w = A.ws + (size_t)seg.dest * A.nb * 512;
            if (has1) {
                double* d = w + ((size_t)c1 * 64 + lane) * 8;
#pragma unroll
                for (int r = 0; r < 8; ++r) d[r] = acc1[r];
            }
            if (has2) {
                double* d = w + ((size_t)c2 * 64 + lane) * 8;
#pragma unroll
                for (int r = 0; r < 8; ++r) d[r] = acc2[r];
            }
        }
    }
#ifdef GFT_TILED_DIAG
    if (A.stamps && tid == 0) A.stamps[3 * (size_t)wg + 1] = __builtin_amdgcn_s_memrealtime();
#endif
    if (!claiming) break;
    }
}

// Fixed-order sum of the partial slabs of split tiles.  One workgroup per (tile, 8-wide output block); its four waves
// each sum a contiguous quarter of the tile's partial slabs and the quarters are added in order through LDS — the order
// depends on the plan only, so results are deterministic.  (A slab step of a recurrence has few tiles and many partial
// slabs: one workgroup per tile walking all of them serially took 140 us at 64^3, 2x the product itself.)
__global__ void __launch_bounds__(256) k_conv_reduce(TiledArgs A, unsigned n_red) {
    const unsigned ti = blockIdx.x, c = blockIdx.y;
    if (ti >= n_red) return;
    if (A.guard && *A.guard == A.guard_epoch) return;
    __shared__ double part[3][64][8];
    const RedTile rt = A.red[ti];
    const unsigned lane = threadIdx.x & 63u, q = threadIdx.x >> 6;
    const unsigned k0 = (64u >> A.tsh) * rt.a + (lane >> A.tsh), k1 = (rt.b << A.tsh) + (lane & ((1u << A.tsh) - 1u));
    bool lane_in = k0 < A.z0 && k1 < A.z1;
    if (A.slab_axis == 1) lane_in = lane_in && k0 >= A.slab_lo && k0 < A.slab_hi;
    else if (A.slab_axis == 2) lane_in = lane_in && k1 >= A.slab_lo && k1 < A.slab_hi;
    double v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = 0.0;
    double* zrow = A.z + A.zoff + (size_t)rt.u * A.zsU + (size_t)k0 * A.zs0 + (size_t)k1 * A.zs1;
    if (lane_in) {
        if (q == 0 && A.accumulate) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                unsigned k2 = 8 * c + r;
                if (k2 < A.zI) v[r] = zrow[k2];
            }
        }
        const unsigned lo = (unsigned)((unsigned long long)rt.count * q / 4), hi = (unsigned)((unsigned long long)rt.count * (q + 1) / 4);
        // (a tile's partial slabs are consecutive workspace slots — the plan's ranges are contiguous in tile order — so
        // the slab address follows from the tile's entry alone: one dependent load less in a launch that is nothing
        // but a few memory latencies; and four slabs' loads go out before the first is added — in the same order as before)
        unsigned p = lo;
        if (!A.red_slots) {
            const size_t stride = (size_t)A.nb * 512;
            const double* w = A.ws + (size_t)(rt.slot0 + lo) * stride + ((size_t)c * 64 + lane) * 8;
            for (; p + 4 <= hi; p += 4, w += 4 * stride) {
                double t[4][8];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int r = 0; r < 8; ++r) t[u][r] = w[(size_t)u * stride + r];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[r] += t[u][r];
            }
        }
        for (; p < hi; ++p) {
            const unsigned slot = A.red_slots ? A.red_slots[rt.first + p] : rt.slot0 + p;
            const double* w = A.ws + (size_t)slot * A.nb * 512 + ((size_t)c * 64 + lane) * 8;
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] += w[r];
        }
        if (q > 0) {
#pragma unroll
            for (int r = 0; r < 8; ++r) part[q - 1][lane][r] = v[r];
        }
    }
    __syncthreads();
    if (q == 0 && lane_in) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] += part[g][lane][r];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            unsigned k2 = 8 * c + r;
            if (k2 < A.zI) zrow[k2] = v[r];
        }
    }
}
// (Round 4 tried 16 waves per (tile, block) with four slabs' loads in flight: 32^3 18 -> 16 us, but 128^3 65 -> 233 us — 60 KB of
// static LDS per workgroup leaves two of them per CU to read 285 MB of slabs.  Kept as it was.)

// out[row][i] = i < len ? in[row][i] : 0, rows x n8
// Operand preparation: rows are copied into the zero-padded packed layout and, on the way, *flag is raised to
// `epoch` if any element is inf/NaN (the verdict is an epoch stamp, so the word never needs resetting).
// Both operands in one launch: x is always packed; y is packed if yp != nullptr, otherwise only scanned.
__global__ void __launch_bounds__(256) k_prep_operands(const double* __restrict__ x, double* __restrict__ xp, size_t x_rows,
                                                       unsigned xlen, unsigned nx8, const double* __restrict__ y,
                                                       double* __restrict__ yp, size_t y_rows, unsigned ylen, unsigned ny8,
                                                       unsigned* flag, unsigned epoch) {
    const size_t tx = x_rows * nx8, ty = yp ? y_rows * ny8 : y_rows * ylen;
    bool bad = false;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < tx + ty; i += (size_t)gridDim.x * blockDim.x) {
        double v;
        if (i < tx) {
            size_t row = i / nx8;
            unsigned col = (unsigned)(i - row * nx8);
            v = col < xlen ? x[row * xlen + col] : 0.0;
            xp[i] = v;
        } else if (yp) {
            size_t k = i - tx, row = k / ny8;
            unsigned col = (unsigned)(k - row * ny8);
            v = col < ylen ? y[row * ylen + col] : 0.0;
            yp[k] = v;
        } else {
            v = y[i - tx];
        }
        if (!((v - v) == 0.0)) bad = true;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicMax(flag, epoch);
}

// Operands of the two leftover products of a peeled n0 x n1 x nI product (conv_tiled_peel), gathered into the packed
// layout (rows of n8 doubles) in one launch:
//   w0[v][a][r1][.]  = x[8a+1+v][r1][.]   window operand of L0, (7, n0/8, n1) rows
//   s1[ju][j1c][.]   = y[j1c][ju][.]      scalar operand of L1, (7, n0) rows
//   w1[v][b][r][.]   = x[r][8b+1+v][.]    window operand of L1, (7, n1/8, n0) rows
// No scan: the main product's k_prep_operands has seen all of x and y.
__global__ void __launch_bounds__(256) k_pack_peel(const double* __restrict__ x, const double* __restrict__ y,
                                                   double* __restrict__ w0, double* __restrict__ s1, double* __restrict__ w1,
                                                   unsigned n0, unsigned n1, unsigned nI, unsigned n8) {
    const size_t t0 = (size_t)7 * (n0 / 8) * n1 * n8, ts = (size_t)7 * n0 * n8, t1 = (size_t)7 * (n1 / 8) * n0 * n8;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < t0 + ts + t1; i += (size_t)gridDim.x * blockDim.x) {
        const double* src;
        double* dst;
        size_t row;
        unsigned col;
        if (i < t0) {
            row = i / n8;
            col = (unsigned)(i - row * n8);
            const unsigned r1 = (unsigned)(row % n1), va = (unsigned)(row / n1), a = va % (n0 / 8), v = va / (n0 / 8);
            src = x + ((size_t)(8 * a + 1 + v) * n1 + r1) * nI;
            dst = w0 + i;
        } else if (i < t0 + ts) {
            const size_t k = i - t0;
            row = k / n8;
            col = (unsigned)(k - row * n8);
            const unsigned j1c = (unsigned)(row % n0), ju = (unsigned)(row / n0);
            src = y + ((size_t)j1c * n1 + ju) * nI;
            dst = s1 + k;
        } else {
            const size_t k = i - t0 - ts;
            row = k / n8;
            col = (unsigned)(k - row * n8);
            const unsigned r = (unsigned)(row % n0), vb = (unsigned)(row / n0), b = vb % (n1 / 8), v = vb / (n1 / 8);
            src = x + ((size_t)r * n1 + 8 * b + 1 + v) * nI;
            dst = w1 + k;
        }
        *dst = col < nI ? src[col] : 0.0;
    }
}

// ---- inner-axis splitting (rank 2, or an inner axis longer than 128) ---------------------------------------------
// A row of length n is viewed as P = ceil(n / B) pieces of B: x~[p][r] = x[pB + r] (zero padded).  The product of
// the (.., Px, B) and (.., Py, B) tensors with an UNtruncated last axis (2B - 1 <= 127 coefficients) contains
// exactly the products of the original one: z[pB + r] = z~[p][r] + z~[p - 1][B + r] (overlap-add of the carries).
// That turns a rank-d product with a long last axis into a rank-(d+1) product the tiled kernel supports.
// Packed layouts put the PIECE axis first — x~[p][row][r], z~[p][row][0..2B-2] — so that the tiled kernel sees it as
// its wave-uniform axis u and the lanes tile real rows (pieces are few: as a lane axis they left most lanes masked).
__global__ void __launch_bounds__(256) k_pad_rows(const double* __restrict__ in, double* __restrict__ out, size_t rows,
                                                  unsigned len, unsigned P, unsigned B) {
    const size_t per_p = rows * B, total = per_p * P;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned p = (unsigned)(i / per_p);
        const size_t rem = i - (size_t)p * per_p, row = rem / B;
        const unsigned col = p * B + (unsigned)(rem - row * B);
        out[i] = col < len ? in[row * len + col] : 0.0;
    }
}
__global__ void __launch_bounds__(256) k_fold_rows(const double* __restrict__ zt, double* __restrict__ z, size_t rows,
                                                   size_t row_lo, size_t row_hi, unsigned Pz, unsigned B, unsigned zI,
                                                   int accumulate, const unsigned* guard, unsigned epoch) {
    if (guard && *guard == epoch) return;
    const unsigned RI = 2 * B - 1;
    size_t total = (row_hi - row_lo) * zI;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t row = row_lo + i / zI;
        unsigned k = (unsigned)(i % zI), p = k / B, r = k - p * B;
        // z~ has Pz = min(pieces of z, pieces of x + pieces of y - 1) pieces: the last output piece may consist of the
        // carry alone (a 110-long row times a 63-long one reaches k = 171 with 2 + 1 - 1 = 2 piece products)
        double v = p < Pz ? zt[((size_t)p * rows + row) * RI + r] : 0.0;
        if (p > 0 && p - 1 < Pz && r + 1 < B) v += zt[((size_t)(p - 1) * rows + row) * RI + B + r];
        double* dst = z + row * zI + k;
        *dst = accumulate ? *dst + v : v;
    }
}

// ---- host-side plan ------------------------------------------------------------------------------------

// ConvArgs::variant (gft_set_conv_variant; -1 = GFT_TILED_DEFAULT_VARIANT) is a bit set.  It is decoded ONCE, at the top
// of conv_tiled_f64, and everything below reads the fields.
struct Variant {
    bool fast;       // 1: software-pipelined fast path for full inner extents
    bool b128;       // 2: ds_read_b128 window loads (even LDS row pitch with P1/2 odd)
    bool xcd;        // 4: XCD-contiguous ranges (the run-time flag TiledArgs::xcd_remap, no instantiation of its own)
    bool compact;    // 8: the pipelined path for compact operands (VAR 11); set by the decoder from the shapes
    bool peel;       // 128: leftover products of a peeled product (VAR 131); set by conv_tiled_peel
    unsigned other;  // 16, 32, 64: timing-only diagnostics (-DGFT_TILED_DIAG, see the VAR bits above); the rest: nothing
};
static_assert((GFT_TILED_DEFAULT_VARIANT & 3) == 3, "only the pipelined b128 kernel (VAR 3) is instantiated for every NW");
// `compact_operands`: x or y spans fewer chunks than z's inner axis, but the fast path (1 | 2) needs both to span every one
Variant decode_variant(int variant, bool compact_operands) {
    if (variant < 0) variant = GFT_TILED_DEFAULT_VARIANT;
    Variant V = {bool(variant & 1), bool(variant & 2), bool(variant & 4), bool(variant & 8), bool(variant & 128),
                 unsigned(variant & ~(1 | 2 | 4 | 8 | 128))};
    if (compact_operands && V.fast && V.b128) V = {true, true, V.xcd, true, false, 0};  // pipelined path for compact operands
    else if (compact_operands) V.fast = V.b128 = false;
    return V;
}
// The VAR of k_conv_tiled that a decoded variant selects on NW waves, or a value that launch_plan does not know.  VAR 131,
// 11, 3 and 0 exist for every NW; the pipelined kernel without b128 (VAR 1) and the diagnostics for NW = 8 only.
int pick_var(const Variant& V, unsigned NW) {
    if (V.peel) return 131;
    if (V.compact) return 11;
    if (V.fast == V.b128 && !V.other) return V.fast ? 3 : 0;
    return (NW == 8 && V.fast && !V.b128 && !V.xcd) ? 1 + (int)V.other : -1;
}

struct PlanKey {
    unsigned v[19];
    bool operator<(const PlanKey& o) const { return std::memcmp(v, o.v, sizeof(v)) < 0; }
};

struct Plan {
    TiledArgs base;  // shapes/pitches filled in; pointers to device tables filled in
    unsigned n_wg = 0, n_red = 0, n_slots = 0, NW = 0;  // n_wg: stream-K ranges (one workgroup each unless the launch claims)
    unsigned n_resident = 0;                            // workgroup slots of the device for this kernel (CUs x workgroups per CU)
    unsigned n_segs = 0;                                // segments of all ranges: n_slots plus the tiles written straight to z
    bool all_slabs = false;                             // PeelSpec::all_slabs: no tile is written straight to z (n_slots == n_segs)
    size_t lds_bytes = 0;
    void* d_tables = nullptr;
};

struct TableArena {
    char* dev = nullptr;
    char* host = nullptr;  // pinned mirror
    size_t bytes = 0, head = 0;
    bool tried = false;
    bool ensure() {
        if (dev) return true;
        if (tried) return false;
        tried = true;
        const size_t n = 32u << 20;
        if (hipMalloc((void**)&dev, n) != hipSuccess) { dev = nullptr; (void)hipGetLastError(); return false; }
        if (hipHostMalloc((void**)&host, n, hipHostMallocDefault) != hipSuccess) {
            (void)hipFree(dev);
            dev = nullptr;
            (void)hipGetLastError();
            return false;
        }
        bytes = n;
        return true;
    }
};
TableArena& arena() {
    static TableArena a;
    return a;
}

std::map<PlanKey, Plan>& plan_cache() {
    static std::map<PlanKey, Plan> c;
    return c;
}

unsigned long long& plan_generation() {  // bumped whenever the plan cache is emptied (cached Plan copies are stale then)
    static unsigned long long g = 0;
    return g;
}

// Drops every cached plan and rewinds the table arena (plans are cheap to rebuild): when the arena wraps, every cached
// plan's slice may be overwritten from then on; and when the cache reaches its bound.
void reset_plan_cache(hipStream_t st) {
    (void)hipStreamSynchronize(st);  // pending uploads still read the host mirror
    for (auto& kv : plan_cache())
        if (kv.second.d_tables) (void)hipFree(kv.second.d_tables);
    plan_cache().clear();
    plan_generation()++;
    arena().head = 0;
}

int num_cus() {
    static int n = 0;
    if (!n) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}

// What distinguishes the three plans of a peeled product from a plain one (all zero: plain).
struct PeelSpec {
    unsigned role = 0;                      // 0 plain, 1 the aligned main part M, 2 / 3 the leftover products L0 / L1
    unsigned cut = 0, lim1 = 0;             // TiledArgs::cut, TiledArgs::lim1
    size_t zsU = 0, zs0 = 0, zs1 = 0, zoff = 0;  // output strides (role 2 / 3; dense otherwise)
    unsigned all_slabs = 0;                 // role 2 / 3 on a lane: every tile goes through a partial slab (the same cuts)
};

int& tiled_slots_cap() {  // A/B and test knob ("tiled_slots"): at most this many workgroups per main launch; 0: one per range or
                          // slot; < 0: one per range whatever the slots (the static launch, A/B)
    static int v = 0;
    return v;
}
// Taper of a claiming plan's ranges, in per cent: along a queue the range sizes fall linearly from (1 + t) to (1 - t)
// times their mean ("tiled_taper", A/B; the default is the sweep's choice, profiles/r18/tiled_taper_sweep.txt)
#ifndef GFT_TILED_TAPER_DEFAULT
#define GFT_TILED_TAPER_DEFAULT 80
#endif
int& tiled_taper_pct() {
    static int v = GFT_TILED_TAPER_DEFAULT;
    return v;
}

int& tiled_force_tsh() {  // A/B and test knob (GFT_TILED_TSH / "tiled_tile"): 3..6 forces the lane tile 8x8 .. 1x64
    static int v = 0;
    return v;
}

// Lane tile: the shape whose lanes are busiest.  A lane (k0, k1) works in step (j0, j1) iff j <= k and k - j < y's
// extent on both axes; the steps a tile runs are the union over its lanes, so a tile straddling the diagonal (or a
// short axis) carries masked lanes.  Useful / issued lane-steps factorises over the two axes.
unsigned pick_lane_tile(const TiledArgs& T) {
    auto axis_eff = [](unsigned T, unsigned nx, unsigned ny, unsigned nz) {
        double useful = 0, issued = 0;
        for (unsigned t = 0; t * T < nz; ++t) {
            const unsigned kmax = std::min(T * t + T - 1, nz - 1);
            const unsigned jlo = T * t + 1 > ny ? T * t + 1 - ny : 0, jhi = std::min(kmax + 1, nx);
            if (jhi > jlo) issued += (double)(jhi - jlo) * T;
            for (unsigned k = T * t; k <= kmax; ++k) {
                const unsigned lo = k + 1 > ny ? k + 1 - ny : 0, hi = std::min(k + 1, nx);
                if (hi > lo) useful += hi - lo;
            }
        }
        return issued > 0 ? useful / issued : 0.0;
    };
    const int force = tiled_force_tsh();
    if (force >= 3 && force <= 6) return (unsigned)force;
    double best = -1.0;
    unsigned best_tsh = 3;
    for (unsigned tsh = 3; tsh <= 6; ++tsh) {
        const double e = axis_eff(64u >> tsh, T.x0, T.y0, T.z0) * axis_eff(1u << tsh, T.x1, T.y1, T.z1);
        if (e > best * 1.02) {  // ties (and near ties) go to the squarer tile: fewer window reloads per step
            best = e;
            best_tsh = tsh;
        }
    }
    return best_tsh;
}

// Which output blocks each wave of a workgroup accumulates (at most two: 16 accumulator VGPR pairs each).
// Block c costs one 8x8x8 chunk product per (x chunk, y chunk) pair that lands in it, i.e. c + 1 for full
// operands.  The classic pairing (c, nb-1-c) gives every ACTIVE wave the same load, but when nb < 2*NW the
// active waves sit unevenly on the CU's four SIMDs (wave w runs on SIMD w % 4): nb = 10 keeps two busy waves on
// SIMD 0 and one on the others, and the whole CU waits for SIMD 0 — measured 62% of the nb = 16 rate.
// Longest-processing-time assignment over SIMDs instead, then over the waves of the SIMD.
void assign_blocks(TiledArgs& T, unsigned NW) {
    for (int w = 0; w < 8; ++w) T.blk1[w] = T.blk2[w] = 0xff;
    // (classic pairs are only balanced when every block c costs c + 1: compact operands — the piece-split products'
    // untruncated inner axis costs min(c + 1, nxc, nyc, nb - c) — always take the LPT assignment)
    const bool full = T.nxc >= T.nb && T.nyc >= T.nb;
    if (full && (2 * NW == T.nb || NW < 4)) {
        for (unsigned w = 0; w < NW; ++w) {
            unsigned c1 = w, c2 = T.nb - 1 - w;
            if (c1 < T.nb && c1 <= c2) T.blk1[w] = (unsigned char)c1;
            if (c2 < T.nb && c2 > c1) T.blk2[w] = (unsigned char)c2;
        }
        return;
    }
    auto cost = [&](unsigned c) {
        unsigned n = 0;
        for (unsigned xc = 0; xc <= c && xc < T.nxc; ++xc)
            if (c - xc < T.nyc) n++;
        return n;
    };
    unsigned simd_load[4] = {0, 0, 0, 0}, wave_load[8] = {0}, wave_cnt[8] = {0};
    for (unsigned i = 0; i < T.nb; ++i) {
        unsigned c = T.nb - 1 - i;  // heaviest first
        int best = -1;
        for (unsigned w = 0; w < NW; ++w) {
            if (wave_cnt[w] >= 2) continue;
            if (best < 0) { best = (int)w; continue; }
            unsigned sb = simd_load[best % 4], sw = simd_load[w % 4];
            if (sw < sb || (sw == sb && wave_load[w] < wave_load[best])) best = (int)w;
        }
        if (wave_cnt[best] == 0) T.blk1[best] = (unsigned char)c;
        else T.blk2[best] = (unsigned char)c;
        wave_cnt[best]++;
        wave_load[best] += cost(c);
        simd_load[best % 4] += cost(c);
    }
}

// Plan step 1: the canonical form z[u][k0][k1][k2] of the problem — u is wave-uniform, (k0, k1) are the lane axes, k2
// the register axis — with its chunk counts, LDS pitch, lane tile, output strides and the waves' output blocks.
// false: the tiled kernel does not take the shape.
bool canonicalise(const ConvArgs& a, const Variant& V, const PeelSpec& ps, Plan& P) {
    TiledArgs& T = P.base;
    std::memset(&T, 0, sizeof(T));
    if (a.slab_axis < 0 || a.slab_axis >= a.nd - 1) return false;
    if (a.nd == 2) {  // rows x inner: no k0 axis — the lane tile becomes 1 x 64 rows
        T.xU = T.yU = T.zU = 1;
        T.x0 = T.y0 = T.z0 = 1;
        T.x1 = a.xs[0]; T.xI = a.xs[1];
        T.y1 = a.ys[0]; T.yI = a.ys[1];
        T.z1 = a.zs[0]; T.zI = a.zs[1];
        T.slab_axis = 2;
    } else if (a.nd == 3) {
        T.xU = T.yU = T.zU = 1;
        T.x0 = a.xs[0]; T.x1 = a.xs[1]; T.xI = a.xs[2];
        T.y0 = a.ys[0]; T.y1 = a.ys[1]; T.yI = a.ys[2];
        T.z0 = a.zs[0]; T.z1 = a.zs[1]; T.zI = a.zs[2];
        T.slab_axis = 1 + (unsigned)a.slab_axis;
    } else if (a.nd == 4) {
        T.xU = a.xs[0]; T.x0 = a.xs[1]; T.x1 = a.xs[2]; T.xI = a.xs[3];
        T.yU = a.ys[0]; T.y0 = a.ys[1]; T.y1 = a.ys[2]; T.yI = a.ys[3];
        T.zU = a.zs[0]; T.z0 = a.zs[1]; T.z1 = a.zs[2]; T.zI = a.zs[3];
        T.slab_axis = (unsigned)a.slab_axis;
    } else {
        return false;
    }
    if (T.zI > 128 || T.xI > T.zI || T.yI > T.zI) return false;
    if (a.j0_min != 0 || a.j0_excl != 0 || a.j0_desc != 0) return false;  // recurrence steps: reference-order kernel
    T.nx8 = (T.xI + 7) / 8 * 8;
    T.ny8 = (T.yI + 7) / 8 * 8;
    T.nxc = T.nx8 / 8;
    T.nyc = T.ny8 / 8;
    T.nb = (T.zI + 7) / 8;
    // front padding + pitch: odd (8-byte slots, bijective mod 16/32 for ds_read_b64/read2_b64) or, for the
    // ds_read_b128 variant, even with P1/2 odd (16-byte slots bijective mod 16 for the b128 lane groups)
    T.P1 = V.b128 ? T.ny8 + YPAD + 2 : T.ny8 + YPAD + 1;
    T.tsh = pick_lane_tile(T);
    // peeled products: the aligned part ends every tile's step range at the tile's first row; the leftover products
    // add into z through their own strides (everything else: dense)
    T.cut = ps.cut;
    T.lim1 = ps.lim1;
    if (ps.role >= 2) {
        T.zsU = ps.zsU; T.zs0 = ps.zs0; T.zs1 = ps.zs1; T.zoff = ps.zoff;
    } else {
        T.zsU = (size_t)T.z0 * T.z1 * T.zI; T.zs0 = (size_t)T.z1 * T.zI; T.zs1 = T.zI; T.zoff = 0;
    }
    T.slab_lo = a.slab_lo;
    T.slab_hi = a.slab_hi;
    T.accumulate = a.accumulate;
    unsigned npairs = (T.nb + 1) / 2;
    P.NW = npairs <= 1 ? 1 : (npairs <= 2 ? 2 : (npairs <= 4 ? 4 : 8));
    P.lds_bytes = (size_t)64 * T.P1 * sizeof(double) + 16;  // the window, and the ticket words of a persistent launch
    assign_blocks(T, P.NW);
    return true;
}

struct PlanTables {  // the host images of a plan's device tables
    std::vector<TileSeg> segs;
    std::vector<unsigned> wg_begin;
    std::vector<RedTile> red;
    std::vector<unsigned> red_slots;
    bool slots_consecutive = true;  // every split tile's pieces are consecutive slots: red_slots is not needed
};

// Plan step 2: the tiles of the slab range in (u, a, b) order, their linearised step space cut into P.n_wg contiguous
// stream-K ranges (segs, wg_begin), and the reduce list of the tiles that a cut splits (red, red_slots).
bool cut_ranges(Plan& P, PlanTables& tb) {
    const TiledArgs& T = P.base;
    const unsigned TT0 = 64u >> T.tsh, TT1 = 1u << T.tsh;
    struct TileInfo { unsigned u, a, b; unsigned long long steps; };
    std::vector<TileInfo> tiles;
    unsigned u_lo = 0, u_hi = T.zU, a_lo = 0, a_hi = (T.z0 + TT0 - 1) / TT0, b_lo = 0, b_hi = (T.z1 + TT1 - 1) / TT1;
    if (T.slab_axis == 0) {
        u_lo = T.slab_lo;
        u_hi = T.slab_hi;
    } else if (T.slab_axis == 1) {
        a_lo = T.slab_lo / TT0;
        a_hi = (T.slab_hi + TT0 - 1) / TT0;
    } else {
        b_lo = T.slab_lo / TT1;
        b_hi = (T.slab_hi + TT1 - 1) / TT1;
    }
    unsigned long long S = 0;
    for (unsigned u = u_lo; u < u_hi; ++u)
        for (unsigned aa = a_lo; aa < a_hi; ++aa)
            for (unsigned bb = b_lo; bb < b_hi; ++bb) {
                TileGeom g = tile_geom(T, T.tsh, u, aa, bb);
                unsigned long long st = (unsigned long long)g.n_ju * g.n_j0 * g.n_j1;
                if (st == 0 || st > 0xffffffffull) return false;
                tiles.push_back({u, aa, bb, st});
                S += st;
            }
    if (tiles.empty()) return false;
    unsigned wg_per_cu = std::min<unsigned>(16u / P.NW, (unsigned)(160 * 1024 / P.lds_bytes));
    if (wg_per_cu < 1) wg_per_cu = 1;
    // Ranges per resident workgroup slot: with exactly one range per slot every workgroup runs from the first to the last
    // cycle of the launch and the slowest (its CU's clock, its neighbours' traffic) sets the time; four ranges per slot let
    // the dispatcher even that out — as many (2, 4, 8) as leave a range >= ~190 steps (128^3: 2312 steps per slot, eight ranges, 27.0 -> 28.7
    // TMAC/s in three alternating runs on one box; 96^3 and 100^3 four, +3 %; 64^3, 81 steps per slot, stays at one: two
    // are neutral, four lose 4 % to the extra partial slabs).
    unsigned long long n_wg = (unsigned long long)num_cus() * wg_per_cu;
    P.n_resident = (unsigned)n_wg;
    const unsigned long long per_slot = S / n_wg;  // steps (one lane tile x one (ju, j0, j1)) per resident slot
    // The leftover products of a peeled product ran on one range per slot at 74 % wave-slot occupancy (their ranges are equal
    // in steps but not in masked lanes; profiles/r18/pmc_tiled_occupancy_parent.json).  The ~190 steps were found on nb = 8
    // (39 units a step, below); the leftover products of the sizes that peel have nb >= 8 and are cut by the same WORK, 190 x 39
    // units a range: 53 steps at nb = 16, two ranges per slot at 128^3, evened out by the persistent launch.
    const bool leftover = T.lim1 || T.zoff;
    const unsigned long long range_steps = leftover ? std::min(190ull, 190ull * 39 / ((unsigned long long)T.nb * (T.nb + 1) / 2 + 3)) : 190;
    const unsigned long long fit = per_slot / range_steps;  // ranges of >= ~190 steps
    n_wg *= fit >= 8 ? 8u : (fit >= 4 ? 4u : (fit >= 2 ? 2u : 1u));
    // Every range pays a window fill and, if it splits a tile, a 4 KB-per-block partial slab plus its share of the
    // reduction, so small products must not be cut into confetti.  A step costs ~ (chunk pairs + 3) units
    // (pairs = nb(nb+1)/2 8x8x8 chunk products per lane tile, 3 ~ barriers + refill) and the fixed part grows
    // with the row length; ranges get >= ~(64 + 20 nb) units (sweep on MI355X: 24^3 171 -> 50 us,
    // 30^3 91 -> 71 us, 10x10x100 154 -> 92 us per product).
    constexpr unsigned long long MIN_UNITS = 64;
    const unsigned long long step_units = (unsigned long long)T.nb * (T.nb + 1) / 2 + 3;
    const unsigned long long min_steps =
        std::max<unsigned long long>(1, (MIN_UNITS + 20ull * T.nb + step_units / 2) / step_units);
    if (n_wg > S / min_steps) n_wg = std::max<unsigned long long>(1, S / min_steps);
    P.n_wg = (unsigned)n_wg;
    // The cuts.  A plan with more ranges than slots is launched persistently (launch_grid) and its ranges TAPER: in each
    // queue (an eighth of the ranges, or all of them: claim_range) the sizes fall linearly from (1 + t) to (1 - t) times the
    // mean, so the ranges claimed last — the launch's tail — are the short ones: a slot that runs out of ranges idles for
    // about half a last range (profiles/r18/tiled_slot_timeline.txt).  t is tiled_taper_pct(), less where the shortest range
    // would drop below the WORK of ~190 steps at nb = 8, where that length was found (tail_steps; what it guards, a
    // range's window fill and its 4 KB-per-block partial slab, is then under 2 % of the range).  Shape and slot count decide
    // all of it: the same cuts whoever runs them.
    std::vector<unsigned long long> cutpos(n_wg + 1);
    for (unsigned long long w = 0; w <= n_wg; ++w) cutpos[w] = S * w / n_wg;
    const unsigned long long mean = S / n_wg;
    const unsigned long long tail_steps = std::max(min_steps, std::min(190ull, 190ull * 39 / step_units));
    if (n_wg > P.n_resident && mean > tail_steps && tiled_taper_pct() > 0) {
        const unsigned nq = n_wg % 8 == 0 ? 8u : 1u;
        const unsigned long long k = n_wg / nq;  // ranges per queue (k >= 2: more ranges than slots)
        const unsigned long long pct = std::min<unsigned long long>(std::min(tiled_taper_pct(), 90), 100 * (mean - tail_steps) / mean);
        // weight of range i of a queue: 100 (k - 1) + pct (k - 1 - 2 i) > 0; the weights of a queue sum to 100 k (k - 1)
        for (unsigned q = 0; q < nq; ++q) {
            const unsigned long long qlo = cutpos[q * k], qS = cutpos[(q + 1) * k] - qlo;
            unsigned long long W = 0;
            for (unsigned long long i = 0; i < k; ++i) {
                cutpos[q * k + i] = qlo + (unsigned long long)((unsigned __int128)qS * W / (100 * k * (k - 1)));
                W += 100 * (k - 1) + pct * (k - 1) - 2 * pct * i;
            }
        }
    }

    tb.wg_begin.assign(P.n_wg + 1, 0);
    std::vector<std::vector<unsigned>> tile_slots(tiles.size());
    std::vector<int> tile_direct(tiles.size(), 0);
    unsigned n_slots = 0;
    size_t ti = 0;
    unsigned long long tile_start = 0;  // global step index where tile ti starts
    for (unsigned w = 0; w < P.n_wg; ++w) {
        unsigned long long lo = cutpos[w], hi = cutpos[w + 1];
        tb.wg_begin[w] = (unsigned)tb.segs.size();
        unsigned long long pos = lo;
        while (pos < hi) {
            while (pos >= tile_start + tiles[ti].steps) {
                tile_start += tiles[ti].steps;
                ti++;
            }
            unsigned long long tend = tile_start + tiles[ti].steps;
            unsigned long long e = hi < tend ? hi : tend;
            TileSeg sg = {tiles[ti].u, tiles[ti].a, tiles[ti].b, (unsigned)(pos - tile_start), (unsigned)(e - tile_start), -1};
            // A tile that one range covers is written straight to z — except by a leftover product of a peeled product that
            // runs on a lane (Plan::all_slabs): its main kernel then runs BESIDE the main part's and the other leftover
            // product's (conv_tiled_peel), which write the same rows of z, so everything it computes goes through a partial
            // slab and reaches z in its reduce, in stream order.  Same bits: the reduce forms ((z + 0) + 0) + (0 + acc) where
            // the direct write forms z + acc, and acc, a chain of fma from +0, is never -0.  (No cut moves; such tiles are
            // the few short ones at the start of each (u, a) run.)
            if (!P.all_slabs && sg.step_begin == 0 && sg.step_end == tiles[ti].steps) {
                tile_direct[ti] = 1;
            } else {
                sg.dest = (int)n_slots;
                tile_slots[ti].push_back(n_slots);
                n_slots++;
            }
            tb.segs.push_back(sg);
            pos = e;
        }
    }
    tb.wg_begin[P.n_wg] = (unsigned)tb.segs.size();
    for (size_t i = 0; i < tiles.size(); ++i) {
        if (tile_direct[i] || tile_slots[i].empty()) continue;
        RedTile r = {tiles[i].u, tiles[i].a, tiles[i].b, (unsigned)tb.red_slots.size(), (unsigned)tile_slots[i].size(), tile_slots[i][0]};
        for (size_t q = 0; q < tile_slots[i].size(); ++q)
            if (tile_slots[i][q] != r.slot0 + q) tb.slots_consecutive = false;
        for (unsigned sl : tile_slots[i]) tb.red_slots.push_back(sl);
        tb.red.push_back(r);
    }
    P.n_red = (unsigned)tb.red.size();
    P.n_slots = n_slots;
    P.n_segs = (unsigned)tb.segs.size();
    return true;
}

// Plan step 3: all tables of a plan live in one slice of a persistent device arena and are uploaded with ONE
// stream-ordered copy from the pinned host mirror of that slice: building a plan for a new shape costs no hipMalloc and
// no host synchronisation (Genfer's supports grow statement by statement, so new shapes are the common case).
bool upload_tables(Plan& P, const PlanTables& tb, hipStream_t st) {
    TiledArgs& T = P.base;
    size_t b_segs = tb.segs.size() * sizeof(TileSeg), b_wg = tb.wg_begin.size() * sizeof(unsigned);
    size_t b_red = tb.red.size() * sizeof(RedTile), b_rs = tb.red_slots.size() * sizeof(unsigned);
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t total = al(b_segs) + al(b_wg) + al(b_red) + al(b_rs) + 256;
    TableArena& A = arena();
    char *base = nullptr, *hbase = nullptr;
    if (A.ensure() && total <= A.bytes / 4) {
        if (A.head + total > A.bytes) reset_plan_cache(st);  // wrap
        base = A.dev + A.head;
        hbase = A.host + A.head;
        A.head += total;
    } else {
        if (hipMalloc(&P.d_tables, total) != hipSuccess) return false;
        base = (char*)P.d_tables;
    }
    size_t off = 0;
    auto put = [&](const void* src, size_t bytes) -> void* {
        void* d = base + off;
        if (bytes) {
            if (hbase) std::memcpy(hbase + off, src, bytes);
            else (void)hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        }
        off += al(bytes);
        return d;
    };
    T.segs = (const TileSeg*)put(tb.segs.data(), b_segs);
    T.wg_begin = (const unsigned*)put(tb.wg_begin.data(), b_wg);
    T.red = (const RedTile*)put(tb.red.data(), b_red);
    T.red_slots = (const unsigned*)put(tb.red_slots.data(), b_rs);
    if (tb.slots_consecutive) T.red_slots = nullptr;  // k_conv_reduce derives the slots from RedTile::slot0
    if (hbase && hipMemcpyAsync(base, hbase, off, hipMemcpyHostToDevice, st) != hipSuccess) return false;
    return true;
}

bool build_plan(const ConvArgs& a, const Variant& V, const PeelSpec& ps, Plan& P, hipStream_t st) {
    PlanTables tb;
    P.all_slabs = ps.all_slabs != 0;
    return canonicalise(a, V, ps, P) && cut_ranges(P, tb) && upload_tables(P, tb, st);
}

template <int NW, int VAR, int TSH>
void launch_main_t(hipStream_t st, const Plan& P, const TiledArgs& T, unsigned grid) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_tiled<NW, VAR, TSH>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_tiled<NW, VAR | 256, TSH>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    // (a failed launch is latched by the launch thread and raised by the next drain: gft_launch.hpp lq_note)
    if (T.claim) GFT_LAUNCH((k_conv_tiled<NW, VAR, TSH>), dim3(grid), dim3(NW * 64), P.lds_bytes, st, T);
    else GFT_LAUNCH((k_conv_tiled<NW, VAR | 256, TSH>), dim3(grid), dim3(NW * 64), P.lds_bytes, st, T);
}
template <int NW, int VAR>
void launch_main_nw(hipStream_t st, const Plan& P, const TiledArgs& T, unsigned grid) {  // the 8x8 lane tile or the run-time one
    if (T.tsh == 3) launch_main_t<NW, VAR, 3>(st, P, T, grid);
    else launch_main_t<NW, VAR, 0>(st, P, T, grid);
}
template <int VAR>
void launch_main(hipStream_t st, const Plan& P, const TiledArgs& T, unsigned grid) {  // the plan's run-time NW as a compile-time one
    switch (P.NW) {
        case 1: launch_main_nw<1, VAR>(st, P, T, grid); break;
        case 2: launch_main_nw<2, VAR>(st, P, T, grid); break;
        case 4: launch_main_nw<4, VAR>(st, P, T, grid); break;
        default: launch_main_nw<8, VAR>(st, P, T, grid); break;
    }
}

}  // namespace

void tiled_pad_rows_f64(hipStream_t st, const double* in, double* out, size_t rows, unsigned len, unsigned P, unsigned B) {
    size_t tot = rows * P * B;
    if (!tot) return;
    GFT_LAUNCH(k_pad_rows, dim3((unsigned)std::min<size_t>((tot + 255) / 256, 4096)), dim3(256), 0, st, in, out, rows,
                       len, P, B);
}
void tiled_fold_rows_f64(hipStream_t st, const double* zt, double* z, size_t rows, size_t row_lo, size_t row_hi, unsigned Pz,
                         unsigned B, unsigned zI, int accumulate, const unsigned* guard, unsigned epoch) {
    size_t tot = (row_hi - row_lo) * zI;
    if (!tot) return;
    GFT_LAUNCH(k_fold_rows, dim3((unsigned)std::min<size_t>((tot + 255) / 256, 4096)), dim3(256), 0, st, zt, z, rows,
                       row_lo, row_hi, Pz, B, zI, accumulate, guard, epoch);
}

void tiled_set_lane_tile(int tsh) { tiled_force_tsh() = tsh; }
void tiled_set_slots(int n) { tiled_slots_cap() = n; }
void tiled_set_taper(int pct) { tiled_taper_pct() = pct < 0 ? GFT_TILED_TAPER_DEFAULT : std::min(pct, 90); }

namespace {

int& tiled_peel_mode() {  // "tiled_peel": -1 auto, 0 never, 1 wherever the structural conditions hold
    static int v = GFT_TILED_PEEL_DEFAULT;
    return v;
}
int& tiled_peel_lanes_mode() {  // "tiled_peel_lanes": 0 a peeled product stays on one stream, 1 its leftover launches take the lanes, -1 by plan
    static int v = GFT_TILED_PEEL_LANES_DEFAULT;
    return v;
}

// The plan of (problem, variant, peel role) from the cache, built on a miss.  The pointer is good until the cache is next
// emptied (plan_generation()); nullptr: the tiled kernel does not support the shape.
const Plan* cached_plan(const ConvArgs& a, const Variant& V, const PeelSpec& ps, hipStream_t st) {
    PlanKey key;
    std::memset(&key, 0, sizeof(key));
    if (a.nd < 2 || a.nd > 4) return nullptr;
    key.v[0] = (unsigned)a.nd | ((unsigned)a.slab_axis << 8) | ((unsigned)tiled_force_tsh() << 16) | ((unsigned)tiled_taper_pct() << 24);
    for (int i = 0; i < a.nd; ++i) {
        key.v[1 + i] = a.xs[i];
        key.v[5 + i] = a.ys[i];
        key.v[9 + i] = a.zs[i];
    }
    key.v[13] = a.slab_lo;
    key.v[14] = a.slab_hi;
    key.v[15] = (unsigned)a.accumulate;
    key.v[16] = (unsigned)(a.j0_min | (a.j0_excl << 8) | (a.j0_desc << 16));
    key.v[17] = V.b128;  // (all a plan takes from the variant is the LDS pitch)
    key.v[18] = ps.role | (ps.cut << 4) | (ps.lim1 << 8) | (ps.all_slabs << 12);  // (the leftover products' output strides follow from role and shapes)
    auto& cache = plan_cache();
    auto it = cache.find(key);
    if (it == cache.end()) {
        Plan P;
        if (cache.size() >= 1024) reset_plan_cache(st);  // bounded
        if (!build_plan(a, V, ps, P, st)) return nullptr;  // may itself reset the cache when the table arena wraps
        it = cache.emplace(key, P).first;
    }
    return &it->second;
}

// Workgroups of plan P's main launch: one per range while they all fit the device's slots at once (the launch every plan
// had before), otherwise one per slot, which then claim the ranges; "tiled_slots" caps it (and never touches the cuts).
unsigned launch_grid(const Plan& P) {
    if (tiled_slots_cap() < 0) return P.n_wg;
    unsigned g = std::min(P.n_wg, P.n_resident);
    if (tiled_slots_cap() > 0) g = std::min(g, (unsigned)tiled_slots_cap());
    return g;
}
bool plan_claims(const Plan& P) { return launch_grid(P) < P.n_wg; }
// The ticket counters of a call's claiming launches: the first CLAIM_BYTES of its workspace, eight words per launch
// (claim_words(0 .. 2): plain or M, L0, L1).  They are zeroed by ONE memset per call, queued in stream order BEFORE the
// launches — not returned to zero by the last workgroup out: the workspace belongs to the stream, not to a plan, and a
// product that does not claim has no counters and puts its partial slabs over these bytes, so "zero on entry" cannot be
// an invariant kept from call to call.  A memset is a node like any other under stream capture, and a launch that the
// non-finite guard stands down never touches the words.
constexpr size_t CLAIM_BYTES = 256;
unsigned* claim_words(char* wb, unsigned launch) { return (unsigned*)wb + 8 * launch; }
void zero_claim_words(hipStream_t st, char* wb) {
    enqueue_task([=] { lq_note((hipMemsetAsync)(wb, 0, CLAIM_BYTES, st), nullptr, "hipMemsetAsync"); });
}

#ifdef GFT_TILED_DIAG
// Timeline (diagnostic build, GFT_TILED_STAMPS=<file>, products whose first launch has at least GFT_TILED_STAMPS_MIN ranges,
// default 1024): every range stamps its start and end in absolute s_memrealtime ticks.  A product has up to three main
// launches (plain: one; peeled: M, L0, L1), each with a stamp area of its own, and ONE dump: per launch and XCD the ranges
// run and when its last range ended relative to the launch's last, and for every launch after the first when its first
// range started and its last ended relative to the FIRST launch's last range end (microseconds at 100 MHz).
// Synchronises: timing runs only.
constexpr unsigned STAMP_RANGES = 65536;
unsigned long long* stamp_area(unsigned launch, const Plan& first) {
    static unsigned long long* d_stamps = nullptr;
    const char* stamps_min = std::getenv("GFT_TILED_STAMPS_MIN");
    if (!std::getenv("GFT_TILED_STAMPS") || first.n_wg < (stamps_min ? (unsigned)std::atoi(stamps_min) : 1024u)) return nullptr;
    if (!d_stamps && hipMalloc((void**)&d_stamps, 3 * (size_t)3 * STAMP_RANGES * sizeof(unsigned long long)) != hipSuccess) d_stamps = nullptr;
    return d_stamps ? d_stamps + (size_t)launch * 3 * STAMP_RANGES : nullptr;
}
struct StampedLaunch {
    const char* name;
    const unsigned long long* d_stamps;
    unsigned n, grid;
    bool claiming;
};
void dump_stamps(hipStream_t st, const StampedLaunch* ls, unsigned n_launches) {
    if (hipStreamSynchronize(st) != hipSuccess) return;
    FILE* f = std::fopen(std::getenv("GFT_TILED_STAMPS"), "a");
    if (!f) return;
    unsigned long long first_end = 0;
    for (unsigned l = 0; l < n_launches; ++l) {
        const unsigned n = ls[l].n;
        std::vector<unsigned long long> h(3 * (size_t)n);
        if (!ls[l].d_stamps || hipMemcpy(h.data(), ls[l].d_stamps, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) continue;
        unsigned long long t0 = ~0ull, t1 = 0, last[8] = {0}, busy[8] = {0};
        unsigned cnt[8] = {0};
        for (unsigned r = 0; r < n; ++r) {
            const unsigned long long b = h[3 * (size_t)r], e = h[3 * (size_t)r + 1];
            const unsigned x = (unsigned)h[3 * (size_t)r + 2] & 7u;
            t0 = std::min(t0, b);
            t1 = std::max(t1, e);
            last[x] = std::max(last[x], e);
            busy[x] += e - b;
            cnt[x]++;
        }
        std::fprintf(f, "launch %s: %u ranges on %u workgroups (%s), %.1f us from first start to last end\n", ls[l].name, n, ls[l].grid,
                     ls[l].claiming ? "claiming" : "one range each", (t1 - t0) / 100.0);
        if (l == 0) first_end = t1;
        else
            std::fprintf(f, "  first range starts %+.1f us, last range ends %+.1f us relative to the last range end of launch %s\n",
                         ((double)t0 - (double)first_end) / 100.0, ((double)t1 - (double)first_end) / 100.0, ls[0].name);
        for (int x = 0; x < 8; ++x)
            std::fprintf(f, "  xcd %d: %5u ranges, range time %10.1f us in all, last range ends %8.1f us before the launch's last\n", x, cnt[x],
                         busy[x] / 100.0, (t1 - last[x]) / 100.0);
    }
    std::fclose(f);
}
#endif

// The main kernel of plan P on the filled-in arguments T, on stream st; `claim`: the launch's ticket counters (used if the
// plan claims).  T leaves with the launch's claim fields set.
bool launch_plan_main(hipStream_t st, const Plan& P, TiledArgs& T, const Variant& V, unsigned* claim) {
    const unsigned grid = launch_grid(P);
    const bool eighths = V.xcd && P.n_wg % 8 == 0;
    T.n_ranges = P.n_wg;
    if (grid < P.n_wg) {
        if (!claim) return false;
        T.claim = claim;
        T.n_queues = eighths ? 8u : 1u;
        T.xcd_remap = 0;
    } else {
        T.claim = nullptr;
        T.n_queues = 1;
        T.xcd_remap = eighths ? 1u : 0u;
    }
#ifdef GFT_TILED_DIAG
    if (P.n_wg > STAMP_RANGES) T.stamps = nullptr;
#endif
    switch (pick_var(V, P.NW)) {
        case 131: launch_main<131>(st, P, T, grid); break;  // leftover products of a peeled product
        case 11: launch_main<11>(st, P, T, grid); break;    // compact operands, pipelined
        case 3: launch_main<3>(st, P, T, grid); break;
        case 0: launch_main<0>(st, P, T, grid); break;
        case 1: launch_main_nw<8, 1>(st, P, T, grid); break;
#ifdef GFT_TILED_DIAG
        case 17: launch_main_nw<8, 17>(st, P, T, grid); break;
        case 33: launch_main_nw<8, 33>(st, P, T, grid); break;
        case 49: launch_main_nw<8, 49>(st, P, T, grid); break;
        case 65: launch_main_nw<8, 65>(st, P, T, grid); break;
        case 113: launch_main_nw<8, 113>(st, P, T, grid); break;
#endif
        default: return false;
    }
    return true;
}
// the fixed-order reduce of plan P's split tiles, on stream st
void launch_plan_reduce(hipStream_t st, const Plan& P, const TiledArgs& T) {
    if (P.n_red) {
        GFT_LAUNCH(k_conv_reduce, dim3(P.n_red, T.nb), dim3(256), 0, st, T, P.n_red);
    }
}
// both on one stream: the plain product
bool launch_plan(hipStream_t st, const Plan& P, TiledArgs T, const Variant& V, unsigned* claim) {
#ifdef GFT_TILED_DIAG
    T.stamps = stamp_area(0, P);
#endif
    if (!launch_plan_main(st, P, T, V, claim)) return false;
#ifdef GFT_TILED_DIAG
    if (T.stamps) {
        const StampedLaunch l = {"plain", T.stamps, P.n_wg, launch_grid(P), plan_claims(P)};
        dump_stamps(st, &l, 1);
    }
#endif
    launch_plan_reduce(st, P, T);
    return true;
}

// How a product's operands reach the kernel, and the common prefix [partial slabs][packed x][packed y] of its workspace.
// Operands are read IN PLACE where their own layout is the packed one: rows of whole chunks (nx8 == xI, ny8 == yI), both
// spanning every chunk of the result's rows (nxc >= nb, nyc >= nb: the compact-operand path multiplies a zero window
// where a block reaches beyond y's last chunk), y 16-byte aligned (window loads are 16-byte), x 8-byte, and 64 readable
// bytes after x's last element (operands_slack: the pipelined path requests one chunk beyond the one it uses; the
// library's own buffers have that slack, a caller's raw pointer may not).  There is then no zero padding anywhere, so
// inf / NaN operands cannot create NaNs the reference does not produce: no verdict, no guarded fallback launch — ONE
// launch per product.  (A peeled product meets the shape part of the condition through peel_applies: full operands.)
// Everything else is packed by k_prep_operands (rows padded to whole chunks plus one chunk of slack after the last row),
// which also takes the non-finite verdict; y alone stays in place if only x needs it.
struct Operands {
    bool inplace, pack_y;
    size_t o_ws, o_xp, o_yp, end;  // byte offsets of the partial slabs (behind the ticket counters of a call that claims) and
                                   // of the packed operands in the workspace, and the end of the common prefix
};
// (sized for the packed layout whether or not this call packs: a query and the launches that follow it — the high-rank
// loop's operand blocks, say — must agree on the workspace whatever their pointers' alignment)
Operands operand_layout(const TiledArgs& B, size_t n_slots, bool claims, const double* x, const double* y, int operands_slack) {
    auto al = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t x_rows = (size_t)B.xU * B.x0 * B.x1, y_rows = (size_t)B.yU * B.y0 * B.y1;
    Operands o;
    o.inplace = operands_slack && B.nx8 == B.xI && B.ny8 == B.yI && B.nxc >= B.nb && B.nyc >= B.nb && !((uintptr_t)y & 15) &&
                !((uintptr_t)x & 7);
    o.pack_y = !o.inplace && (B.ny8 != B.yI || ((uintptr_t)y & 15));
    o.o_ws = claims ? CLAIM_BYTES : 0;
    o.o_xp = o.o_ws + al(n_slots * B.nb * 512 * sizeof(double));
    o.o_yp = o.o_xp + al((x_rows * B.nx8 + 8) * sizeof(double));
    o.end = o.o_yp + al(y_rows * B.ny8 * sizeof(double));
    return o;
}
// Binds x and y to T as the layout says: in place, or packed into the workspace `wb` under the verdict (nf_flag, nf_epoch).
void bind_operands(hipStream_t st, const Operands& o, const double* x, const double* y, char* wb, unsigned* nf_flag,
                   unsigned nf_epoch, TiledArgs& T) {
    T.ws = (double*)(wb + o.o_ws);
    if (o.inplace) {
        T.xp = x;
        T.yp = y;
        T.guard = nullptr;
        T.guard_epoch = 0;
        return;
    }
    const size_t x_rows = (size_t)T.xU * T.x0 * T.x1, y_rows = (size_t)T.yU * T.y0 * T.y1;
    double *xp = (double*)(wb + o.o_xp), *yp = (double*)(wb + o.o_yp);
    const size_t tot = x_rows * T.nx8 + (o.pack_y ? y_rows * T.ny8 : y_rows * T.yI);
    GFT_LAUNCH(k_prep_operands, dim3((unsigned)std::min<size_t>((tot + 255) / 256, 2048)), dim3(256), 0, st, x, xp, x_rows, T.xI,
               T.nx8, y, o.pack_y ? yp : nullptr, y_rows, T.yI, T.ny8, nf_flag, nf_epoch);
    T.xp = xp;
    T.yp = o.pack_y ? yp : y;
    T.guard = nf_flag;
    T.guard_epoch = nf_epoch;
}

// Does the product take the peel?  Structural conditions: rank 3, the whole slab range, operands as large as the result
// on every axis, both lane axes whole 8-row tiles (at least two), the pipelined full-extent kernel on the 8x8 lane
// tile.  Auto mode adds the size threshold: the leftover products' batch axis (n / 8 tiles) must fill the eight lanes
// of its lane-tile axis, and the two extra launches and their partial slabs must be worth the masks they remove
// (PEEL_MIN_EXTENT, PEEL_MIN_INNER: profiles/r07/tiled_peel_sweep.txt).
bool peel_applies(const ConvArgs& a, const Variant& V) {
    const int mode = tiled_peel_mode();
    if (mode == 0) return false;
    if (a.nd != 3 || a.slab_axis != 0 || a.slab_lo != 0 || a.slab_hi != a.zs[0]) return false;
    if (a.j0_min || a.j0_excl || a.j0_desc) return false;
    for (int i = 0; i < 3; ++i)
        if (a.xs[i] != a.zs[i] || a.ys[i] != a.zs[i]) return false;
    const unsigned n0 = a.zs[0], n1 = a.zs[1];
    if (n0 % 8 || n1 % 8 || n0 < 16 || n1 < 16 || a.zs[2] > 128) return false;
    if (!V.fast || !V.b128 || V.compact || V.peel || V.other) return false;  // (external 3 or 7)
    TiledArgs T;
    std::memset(&T, 0, sizeof(T));
    T.x0 = T.y0 = T.z0 = n0;
    T.x1 = T.y1 = T.z1 = n1;
    if (pick_lane_tile(T) != 3) return false;
    return mode == 1 || (n0 >= PEEL_MIN_EXTENT && n1 >= PEEL_MIN_EXTENT && a.zs[2] >= PEEL_MIN_INNER);
}

// A peeled product  z (+)= x (*) y  of full n0 x n1 x nI operands on the 8x8 lane tile.  With a = k0 / 8, b = k1 / 8 a
// term pair (j0, k0) of axis 0 is ALIGNED if j0 <= 8a and a LEFTOVER if 8a < j0 <= k0 (the 28-pair triangle of tile a),
// likewise on axis 1, and the term set aligned x aligned  u  leftover0 x all1  u  aligned0 x leftover1 is computed as
//   M    the plain kernel with every tile's step range cut to j0 <= 8a, j1 <= 8b: no masked lane;
//   L0   rank 4 (u = m, k0c = a, k1c = k1, k2):  z[8a+1+m][k1] += sum_{ju <= m} y[ju][j1] x[8a+1+m-ju][k1-j1] — the
//        scalar operand is y's first seven slabs as they stand, the window operand the gathered slabs of x; u is the
//        wave-uniform axis (no masks), the tile index a a pure batch axis;
//   L1   rank 4 (u = m, k0c = b, k1c = k0, k2):  z[k0][8b+1+m] += sum_{ju <= m, j} y[j][ju] x[k0-j][8b+1+m-ju] with the
//        aligned restriction k0 - j <= 8 (k0 / 8) as a per-lane limit on the window row (TiledArgs::lim1).
// z is written in a fixed order, all on the product's stream: M and its reduce, L0 and its reduce, L1 and its reduce —
// deterministic.  With "tiled_peel_lanes" the leftover products run on plans whose MAIN kernels write nothing but partial
// slabs (PeelSpec::all_slabs: the same cuts, no tile straight to z) into regions of their own, and read only the operands
// and what k_pack_peel gathered; those main kernels are issued on the library's two lanes (gft_launch.hpp) beside M: forked
// behind the pack, joined before L0's reduce, and they fill the wave slots that M's workgroups leave as M's queues run dry
// (DESIGN 3.1).  z is still written by M, M's reduce, L0's reduce, L1's reduce in that order, and the bits are the same
// (cut_ranges).  No fork while the stream is being captured, without lanes, or with the option off: then the launches, the
// plans and their order are what they were without lanes.  All three carry the same guard, so a product flagged non-finite
// is left to the caller's guarded reference-order launch as a whole.
// Workspace: gft_peel_layout.hpp — ONE layout, forked or not: the leftover launches' slab regions are sized for a slab per
// segment (Plan::n_segs, which both kinds of plan share), so a query and the launches after it agree whatever they decide.
// Returns 1 done (or, for a query, sized), 0 a launch failed, -1 the peel cannot be planned or does not fit the workspace
// it was given — nothing has been launched and the caller takes the plain plan.
int conv_tiled_peel(hipStream_t st, const double* x, const double* y, double* z, const ConvArgs& a, const Variant& V, void* ws,
                    size_t ws_bytes, size_t* ws_needed, unsigned* nf_flag, unsigned nf_epoch, bool* guarded, bool* forked) {
    const unsigned n0 = a.zs[0], n1 = a.zs[1], nI = a.zs[2];
    ConvArgs l0, l1;
    std::memset(&l0, 0, sizeof(l0));
    l0.nd = 4;
    l0.slab_lo = 0;
    l0.slab_hi = 7;
    l0.accumulate = 1;
    l1 = l0;
    Variant VL = V;  // the leftover products: the peel instantiation
    VL.peel = true;
    const unsigned s0x[4] = {7, 1, n1, nI}, s0y[4] = {7, n0 / 8, n1, nI}, s1x[4] = {7, 1, n0, nI}, s1y[4] = {7, n1 / 8, n0, nI};
    for (int i = 0; i < 4; ++i) {
        l0.xs[i] = s0x[i]; l0.ys[i] = l0.zs[i] = s0y[i];
        l1.xs[i] = s1x[i]; l1.ys[i] = l1.zs[i] = s1y[i];
    }
    const int lanes_mode = tiled_peel_lanes_mode();
    bool can_fork = lanes_mode != 0 && stream_lanes().ok;
    if (can_fork) {  // (a captured graph with parallel branches is fragile where hardware queues are few)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
        if (cs != hipStreamCaptureStatusNone) can_fork = false;
    }
    bool fork = can_fork && lanes_mode > 0;
    PeelSpec pm, p0, p1;
    pm.role = 1; pm.cut = 3;
    p0.role = 2; p0.zsU = (size_t)n1 * nI; p0.zs0 = 8 * p0.zsU; p0.zs1 = nI; p0.zoff = p0.zsU;
    p1.role = 3; p1.lim1 = 1; p1.zsU = nI; p1.zs0 = 8 * (size_t)nI; p1.zs1 = (size_t)n1 * nI; p1.zoff = nI;
    Plan PM, P0, P1;  // copies: building one plan may empty the cache the others came from (then once more, from an empty arena)
    for (int attempt = 0;; ++attempt) {
        const unsigned long long gen = plan_generation();
        const Plan* q = cached_plan(a, V, pm, st);
        if (!q) return -1;
        PM = *q;
        for (int pass = 0; pass < 2; ++pass) {
            p0.all_slabs = p1.all_slabs = fork ? 1u : 0u;
            if (!(q = cached_plan(l0, VL, p0, st))) return -1;
            P0 = *q;
            if (!(q = cached_plan(l1, VL, p1, st))) return -1;
            P1 = *q;
            // By default the lanes are for leftover launches that are persistent by themselves (more ranges than slots: from
            // 128^3): those fill M's tail and each other's.  Static ones — one short range per workgroup, 112^3, 128 x 128 x 64
            // — gain nothing there and pay the fork, the join and their all-slabs reduces: 1.6 - 2 % slower
            // (profiles/r21/tiled_peel_lanes_sweep.txt).  The cuts, hence the answer, are the same for both kinds of plan.
            if (fork || !can_fork || !(plan_claims(P0) && plan_claims(P1))) break;
            fork = true;
        }
        if (gen == plan_generation()) break;
        if (attempt) return -1;
    }
    const TiledArgs& B = PM.base;
    if (B.tsh != 3) return -1;
    const bool claims = plan_claims(PM) || plan_claims(P0) || plan_claims(P1);
    Operands o = operand_layout(B, 0, claims, x, y, a.operands_slack);  // (in place or packed; the offsets are the peel layout's)
    const size_t slots[3] = {PM.n_slots, P0.n_segs, P1.n_segs};
    const PeelLayout L = peel_layout_for(slots, n0, n1, B.nx8, claims);
    o.o_ws = L.o_slab[0];
    o.o_xp = L.o_xp;
    o.o_yp = L.o_yp;
    if (ws && ws_bytes < L.need) return -1;  // (sized by a query that could not plan the peel)
    if (ws_needed) *ws_needed = L.need;
    if (guarded) *guarded = !o.inplace;
    if (!ws) return 1;  // query

    const hipStream_t st0 = fork ? stream_lanes().st[0] : st, st1 = fork ? stream_lanes().st[1] : st;
    if (forked) *forked = fork;

    char* wb = (char*)ws;
    double *w0 = (double*)(wb + L.o_w0), *s1 = (double*)(wb + L.o_s1), *w1 = (double*)(wb + L.o_w1);
    TiledArgs T = B;
    // the ticket words, the guard word (k_prep_operands) and the gathered operands: all before the fork, the lanes see them
    if (claims) zero_claim_words(st, wb + L.o_claim);
    bind_operands(st, o, x, y, wb, nf_flag, nf_epoch, T);
    {
        const size_t tot = L.b_w0 / sizeof(double) + (L.b_s1 / sizeof(double) - 8) + L.b_w1 / sizeof(double);
        GFT_LAUNCH(k_pack_peel, dim3((unsigned)std::min<size_t>((tot + 255) / 256, 4096)), dim3(256), 0, st, x, y, w0, s1, w1, n0, n1,
                   nI, B.nx8);
    }
    if (fork) lanes_fork(st);
    T.z = z;
    TiledArgs T0 = P0.base, T1 = P1.base;
    T0.ws = (double*)(wb + L.o_slab[1]);
    T1.ws = (double*)(wb + L.o_slab[2]);
    T0.z = T1.z = z;
    T0.guard = T1.guard = T.guard;
    T0.guard_epoch = T1.guard_epoch = T.guard_epoch;
    T0.xp = T.yp;  // y's first seven slabs, in the layout the main launch reads them in (the eighth is the slack)
    T0.yp = w0;
    T1.xp = s1;
    T1.yp = w1;
#ifdef GFT_TILED_DIAG
    T.stamps = stamp_area(0, PM);
    T0.stamps = stamp_area(1, PM);
    T1.stamps = stamp_area(2, PM);
#endif
    unsigned *const c = claim_words(wb + L.o_claim, 0), *const c0 = claim_words(wb + L.o_claim, 1), *const c1 = claim_words(wb + L.o_claim, 2);
    if (fork) {
        // M first: of the launches pending at the fork it is the one the dispatcher should see first
        const bool ok = launch_plan_main(st, PM, T, V, c) && launch_plan_main(st0, P0, T0, VL, c0) && launch_plan_main(st1, P1, T1, VL, c1);
        if (ok) launch_plan_reduce(st, PM, T);
        lanes_join(st);  // (also after a failed launch: the lanes never stay forked)
        if (!ok) return 0;
        launch_plan_reduce(st, P0, T0);
        launch_plan_reduce(st, P1, T1);
    } else {  // one stream: a leftover launch may write tiles straight to z, so each follows the reduce before it
        if (!launch_plan_main(st, PM, T, V, c)) return 0;
        launch_plan_reduce(st, PM, T);
        if (!launch_plan_main(st, P0, T0, VL, c0)) return 0;
        launch_plan_reduce(st, P0, T0);
        if (!launch_plan_main(st, P1, T1, VL, c1)) return 0;
        launch_plan_reduce(st, P1, T1);
    }
#ifdef GFT_TILED_DIAG
    if (T.stamps) {
        const StampedLaunch ls[3] = {{"M", T.stamps, PM.n_wg, launch_grid(PM), plan_claims(PM)},
                                     {"L0", T0.stamps, P0.n_wg, launch_grid(P0), plan_claims(P0)},
                                     {"L1", T1.stamps, P1.n_wg, launch_grid(P1), plan_claims(P1)}};
        dump_stamps(st, ls, 3);
    }
#endif
    return 1;
}

}  // namespace

void tiled_set_peel(int mode) { tiled_peel_mode() = mode < 0 ? -1 : (mode ? 1 : 0); }
void tiled_set_peel_lanes(int mode) { tiled_peel_lanes_mode() = mode < 0 ? GFT_TILED_PEEL_LANES_DEFAULT : (mode ? 1 : 0); }  // (< 0: the default, by plan)

bool conv_tiled_f64(hipStream_t st, const double* x, const double* y, double* z, const ConvArgs& a, void* ws, size_t ws_bytes,
                    size_t* ws_needed, unsigned* nf_flag, unsigned nf_epoch, bool* guarded, bool* peeled, bool* forked) {
    bool compact_operands = false;
    if (a.nd >= 2 && a.nd <= 4) {
        const unsigned nb = (a.zs[a.nd - 1] + 7) / 8;
        compact_operands = (a.xs[a.nd - 1] + 7) / 8 < nb || (a.ys[a.nd - 1] + 7) / 8 < nb;
    }
    const Variant V = decode_variant(a.variant, compact_operands);
    if (peeled) *peeled = false;
    if (forked) *forked = false;
    if (peel_applies(a, V)) {
        const int r = conv_tiled_peel(st, x, y, z, a, V, ws, ws_bytes, ws_needed, nf_flag, nf_epoch, guarded, forked);
        if (r >= 0) {
            if (peeled) *peeled = r == 1;
            return r == 1;
        }
        // (the peel could not be planned: the plain plan below, for the query and for the launch alike)
    }
    const Plan* P = cached_plan(a, V, PeelSpec(), st);
    if (!P) return false;
    const bool claims = plan_claims(*P);
    const Operands o = operand_layout(P->base, P->n_slots, claims, x, y, a.operands_slack);
    const size_t need = o.end + 256;  // workspace: [ticket counters, if the launch claims][partial slabs][packed x][packed y]
    if (guarded) *guarded = !o.inplace;
    if (ws_needed) *ws_needed = need;
    if (!ws) return true;  // query
    if (ws_bytes < need) return false;
    TiledArgs T = P->base;
    if (claims) zero_claim_words(st, (char*)ws);
    bind_operands(st, o, x, y, (char*)ws, nf_flag, nf_epoch, T);
    T.z = z;
    return launch_plan(st, *P, T, V, claim_words((char*)ws, 0));
}

}  // namespace gft
