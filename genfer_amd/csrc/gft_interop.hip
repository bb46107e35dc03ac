// Device interop kernels: bit copies between a caller's strided device tensor and a handle's compact buffer
// (gft_from_device / gft_to_device, gft_interop.hpp).  The elements move as 64-bit integers: no arithmetic touches them,
// so -0.0, NaN payloads, infinities and subnormals arrive as they left.  Plain C++ loads and stores only.
//
// Three forms, chosen on the host per call (interop_copy):
//   dense  both sides C-contiguous after merging (planes back to back): one flat copy, 16 bytes per lane when both
//          pointers allow it;
//   rows   the last axis is the fastest on both sides (or the strided side repeats it, stride 0): a group of lanes per
//          row, loads and stores along the row, the outer index decomposed once per row;
//   tile   the strided side's fastest axis is another one (a permute / .t() view): 64 x 64 tiles staged through LDS so
//          that the reads run along one side's fastest axis and the writes along the other's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "gft_interop.hpp"

namespace gft {

namespace {

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr int IO_THREADS = 256;
constexpr size_t IO_MAX_BLOCKS = 256 * 32;  // grid-stride loops above this (256 CUs, 8 blocks of 4 waves each per SIMD set)
constexpr int TILE = 64;
constexpr int TILE_PITCH = TILE + 1;  // odd pitch in doubles: a column read by ds_read_b64 hits 32 distinct bank pairs per half-wave

struct RowsArgs {
    int nd;
    int narrow;  // every outer index fits 32 bits: the per-row decomposition uses 32-bit division
    size_t nrows;
    size_t nch, chunk;  // a row is cut into nch pieces of `chunk` elements (long rows: more groups than rows)
    size_t ext[IMAXD], ss[IMAXD], ds[IMAXD];
};

struct TileArgs {
    int nout;  // outer axes (every axis but A and B)
    size_t oext[IMAXD], oss[IMAXD], ods[IMAXD];
    size_t extA, extB;    // A: the source's fastest axis (reads run along it), B: the destination's (writes run along it)
    size_t sA, sB, dA, dB;
    size_t nTA, nTB, ntiles;
};

// n elements, src and dst both contiguous.  VEC: both 16-byte aligned, two elements per load / store.
template <bool VEC>
__global__ __launch_bounds__(IO_THREADS) void k_io_dense(const u64* __restrict__ src, u64* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * IO_THREADS;
    size_t i = (size_t)blockIdx.x * IO_THREADS + threadIdx.x;
    if (VEC) {
        const u64x2* s = reinterpret_cast<const u64x2*>(src);
        u64x2* d = reinterpret_cast<u64x2*>(dst);
        const size_t n2 = n / 2;
        for (; i + 3 * stride < n2; i += 4 * stride) {  // four 16-byte loads in flight per lane
            const u64x2 v0 = s[i], v1 = s[i + stride], v2 = s[i + 2 * stride], v3 = s[i + 3 * stride];
            d[i] = v0;
            d[i + stride] = v1;
            d[i + 2 * stride] = v2;
            d[i + 3 * stride] = v3;
        }
        for (; i < n2; i += stride) d[i] = s[i];
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = src[n - 1];
    } else {
        for (; i + 3 * stride < n; i += 4 * stride) {
            const u64 v0 = src[i], v1 = src[i + stride], v2 = src[i + 2 * stride], v3 = src[i + 3 * stride];
            dst[i] = v0;
            dst[i + stride] = v1;
            dst[i + 2 * stride] = v2;
            dst[i + 3 * stride] = v3;
        }
        for (; i < n; i += stride) dst[i] = src[i];
    }
}

// One group of G = 2^LG lanes per row of the last axis; groups stride over the rows.
template <int LG>
__global__ __launch_bounds__(IO_THREADS) void k_io_rows(const u64* __restrict__ src, u64* __restrict__ dst, RowsArgs a) {
    constexpr int G = 1 << LG;
    constexpr int GPB = IO_THREADS / G;  // groups per block
    const size_t lane = threadIdx.x & (G - 1);
    const int last = a.nd - 1;
    const size_t L = a.ext[last], sl = a.ss[last], dl = a.ds[last];
    const size_t items = a.nrows * a.nch;
    for (size_t w = (size_t)blockIdx.x * GPB + (threadIdx.x >> LG); w < items; w += (size_t)gridDim.x * GPB) {
        const size_t r = a.nch == 1 ? w : w / a.nch;
        const size_t j0 = (w - r * a.nch) * a.chunk;
        const size_t jend = L - j0 < a.chunk ? L : j0 + a.chunk;
        size_t so = 0, dof = 0;
        if (a.narrow) {
            unsigned q = (unsigned)r;
            for (int ax = last - 1; ax >= 0; --ax) {
                const unsigned e = (unsigned)a.ext[ax], nq = q / e, k = q - nq * e;
                q = nq;
                so += (size_t)k * a.ss[ax];
                dof += (size_t)k * a.ds[ax];
            }
        } else {
            size_t q = r;
            for (int ax = last - 1; ax >= 0; --ax) {
                const size_t e = a.ext[ax], nq = q / e, k = q - nq * e;
                q = nq;
                so += k * a.ss[ax];
                dof += k * a.ds[ax];
            }
        }
        const u64* s = src + so;
        u64* d = dst + dof;
        size_t j = j0 + lane;
        for (; j + 3 * G < jend; j += 4 * G) {
            const u64 v0 = s[j * sl], v1 = s[(j + G) * sl], v2 = s[(j + 2 * G) * sl], v3 = s[(j + 3 * G) * sl];
            d[j * dl] = v0;
            d[(j + G) * dl] = v1;
            d[(j + 2 * G) * dl] = v2;
            d[(j + 3 * G) * dl] = v3;
        }
        for (; j < jend; j += G) d[j * dl] = s[j * sl];
    }
}

// 64 x 64 tiles over (A, B).  Reads: lane x along A (the source's fastest axis), 4 waves x 16 steps along B, into tile[b][a].
// Writes: lane x along B (the destination's fastest axis), reading the tile's column tile[x][a] — pitch 65 doubles, so the
// 32 lanes of a ds_read_b64 half-wave touch 32 distinct bank pairs.
__global__ __launch_bounds__(IO_THREADS) void k_io_tile(const u64* __restrict__ src, u64* __restrict__ dst, TileArgs a) {
    __shared__ u64 tile[TILE * TILE_PITCH];
    const int x = threadIdx.x & (TILE - 1), y = threadIdx.x / TILE;
    constexpr int STEPS = TILE / (IO_THREADS / TILE);
    for (size_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        size_t q = t;
        const size_t tb = q % a.nTB;
        q /= a.nTB;
        const size_t ta = q % a.nTA;
        q /= a.nTA;
        size_t so = 0, dof = 0;
        for (int ax = a.nout - 1; ax >= 0; --ax) {  // once per tile
            const size_t e = a.oext[ax], nq = q / e, k = q - nq * e;
            q = nq;
            so += k * a.oss[ax];
            dof += k * a.ods[ax];
        }
        const size_t a0 = ta * TILE, b0 = tb * TILE;
        const size_t na = a.extA - a0 < (size_t)TILE ? a.extA - a0 : (size_t)TILE;
        const size_t nb = a.extB - b0 < (size_t)TILE ? a.extB - b0 : (size_t)TILE;
        {
            const u64* s = src + so + (a0 + x) * a.sA + b0 * a.sB;
            u64 v[STEPS];
#pragma unroll
            for (int k = 0; k < STEPS; ++k) {
                const int b = y + k * (IO_THREADS / TILE);
                if ((size_t)x < na && (size_t)b < nb) v[k] = s[(size_t)b * a.sB];
            }
#pragma unroll
            for (int k = 0; k < STEPS; ++k) {
                const int b = y + k * (IO_THREADS / TILE);
                if ((size_t)x < na && (size_t)b < nb) tile[b * TILE_PITCH + x] = v[k];
            }
        }
        __syncthreads();
        {
            u64* d = dst + dof + a0 * a.dA + (b0 + x) * a.dB;
#pragma unroll
            for (int k = 0; k < STEPS; ++k) {
                const int aa = y + k * (IO_THREADS / TILE);
                if ((size_t)x < nb && (size_t)aa < na) d[(size_t)aa * a.dA] = tile[x * TILE_PITCH + aa];
            }
        }
        __syncthreads();
    }
}

static unsigned grid_for(size_t work_items, size_t per_block) {
    size_t b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > IO_MAX_BLOCKS) b = IO_MAX_BLOCKS;
    return (unsigned)b;
}

// fastest axis (smallest non-zero stride; the later axis on a tie), -1 if every stride is 0
static int fastest(const size_t* st, int nd) {
    int best = -1;
    for (int a = 0; a < nd; ++a)
        if (st[a] != 0 && (best < 0 || st[a] <= st[best])) best = a;
    return best;
}

}  // namespace

int interop_copy(hipStream_t st, const double* src_d, double* dst_d, const CopyGeom& in) {
    const u64* src = reinterpret_cast<const u64*>(src_d);
    u64* dst = reinterpret_cast<u64*>(dst_d);
    // unit axes go, axes contiguous with their inner neighbour on both sides merge
    CopyGeom g;
    g.nd = 0;
    for (int a = 0; a < in.nd; ++a) {
        if (in.ext[a] == 1) continue;
        if (g.nd > 0) {
            const int p = g.nd - 1;
            if (g.ss[p] == in.ss[a] * in.ext[a] && g.ds[p] == in.ds[a] * in.ext[a]) {
                g.ext[p] *= in.ext[a];
                g.ss[p] = in.ss[a];
                g.ds[p] = in.ds[a];
                continue;
            }
        }
        g.ext[g.nd] = in.ext[a];
        g.ss[g.nd] = in.ss[a];
        g.ds[g.nd] = in.ds[a];
        ++g.nd;
    }
    if (g.nd == 0) {  // one element
        g.nd = 1;
        g.ext[0] = 1;
        g.ss[0] = g.ds[0] = 1;
    }
    const int nd = g.nd;
    if (nd == 1 && g.ss[0] == 1 && g.ds[0] == 1) {
        const size_t n = g.ext[0];
        if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16 == 0)
            GFT_LAUNCH(k_io_dense<true>, dim3(grid_for(n / 2, IO_THREADS * 4)), dim3(IO_THREADS), 0, st, src, dst, n);
        else
            GFT_LAUNCH(k_io_dense<false>, dim3(grid_for(n, IO_THREADS * 4)), dim3(IO_THREADS), 0, st, src, dst, n);
        return IO_DENSE;
    }
    if (nd > IMAXD) throw std::runtime_error("device interop: the tensor has more than " + std::to_string(IMAXD) + " non-contiguous axes");
    const int A = fastest(g.ss, nd), B = fastest(g.ds, nd);
    if (A >= 0 && B >= 0 && A != B && g.ext[A] >= 16 && g.ext[B] >= 16) {
        TileArgs t;
        t.nout = 0;
        size_t outer = 1;
        for (int a = 0; a < nd; ++a) {
            if (a == A || a == B) continue;
            t.oext[t.nout] = g.ext[a];
            t.oss[t.nout] = g.ss[a];
            t.ods[t.nout] = g.ds[a];
            ++t.nout;
            outer *= g.ext[a];
        }
        t.extA = g.ext[A];
        t.extB = g.ext[B];
        t.sA = g.ss[A];
        t.sB = g.ss[B];
        t.dA = g.ds[A];
        t.dB = g.ds[B];
        t.nTA = (t.extA + TILE - 1) / TILE;
        t.nTB = (t.extB + TILE - 1) / TILE;
        t.ntiles = outer * t.nTA * t.nTB;
        GFT_LAUNCH(k_io_tile, dim3(grid_for(t.ntiles, 1)), dim3(IO_THREADS), 0, st, src, dst, t);
        return IO_TILE;
    }
    RowsArgs r;
    r.nd = nd;
    r.nrows = 1;
    for (int a = 0; a < nd; ++a) {
        r.ext[a] = g.ext[a];
        r.ss[a] = g.ss[a];
        r.ds[a] = g.ds[a];
        if (a < nd - 1) r.nrows *= g.ext[a];
    }
    r.narrow = r.nrows <= 0xffffffffull;
    const size_t L = g.ext[nd - 1];
    int lg = 2;  // lanes per row: the smallest power of two >= the row, 4 .. 64
    while (lg < 6 && ((size_t)1 << lg) < L) ++lg;
    r.chunk = ((size_t)1 << lg) * 16;
    r.nch = (L + r.chunk - 1) / r.chunk;
    const size_t rows_per_block = (size_t)IO_THREADS >> lg;
    const dim3 grid(grid_for(r.nrows * r.nch, rows_per_block)), block(IO_THREADS);
    switch (lg) {
        case 2: GFT_LAUNCH(k_io_rows<2>, grid, block, 0, st, src, dst, r); break;
        case 3: GFT_LAUNCH(k_io_rows<3>, grid, block, 0, st, src, dst, r); break;
        case 4: GFT_LAUNCH(k_io_rows<4>, grid, block, 0, st, src, dst, r); break;
        case 5: GFT_LAUNCH(k_io_rows<5>, grid, block, 0, st, src, dst, r); break;
        default: GFT_LAUNCH(k_io_rows<6>, grid, block, 0, st, src, dst, r); break;
    }
    return IO_ROWS;
}

}  // namespace gft
