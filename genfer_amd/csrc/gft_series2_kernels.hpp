// Device side of the batched bivariate series (gft_series2.hip plans and launches these).  One workgroup is one item
// for the whole operation, the operands resident in LDS.  tests/series2_isa_check.hip instantiates the kernels from this file.
//
// An item is an [n0, n1] coefficient array, axis 0 the rows.  Every operation is the reference's recursion over axis 0 whose
// terms are univariate products of rows, mul_1d(a, b)[k1] = 0.0 + sum_{j1} a[j1] * b[k1 - j1] (ascending j1, stored
// coefficients only), added in ascending j to the accumulator of row k: "independent row sums, ordered additions".
//   mul            a thread owns whole outputs (k0, k1) and runs both sums; no step depends on another.
//   compose        the Horner loop over the slices of f along the substituted axis, every step that product at the compact shape
//                  of the step, the result resident in LDS from step to step (k_series2_compose).
//   div, exp, log  rows k one after the other.  Pass 1 forms the row sums of a chunk of j in parallel over (j, k1) into an LDS
//                  scratch of `srows` rows, pass 2 adds them in ascending j into r[k] (which holds the accumulator between
//                  chunks); then the row's own step: negate and add the dividend, the 1-d division by row 0 of the divisor, the
//                  division by k.  Chunking changes how many row sums are in flight, never the order of an addition.
//   corr           mul transposed: both sums descending, so an output is mul's on the flipped array, which is how g is staged
//                  (k_series2_corr).
//   compose_adj    compose's loop transposed: every step that corr at the compact shapes of the forward loop run backwards
//                  (k_series2_compose_adj).  Both F64 only, and templates so that only gft_series2.hip emits them.
// Multiply and add are rounded separately (-ffp-contract=off) and no explicit fma is written.
//
// The bodies are templates over the element functor (gft_elem.hpp).  k_series2_mul, k_series2_rec<OP> and k_series2_compose<GLDS> are
// the EF64 kernels; k_series2i_mul<E>, k_series2i_rec<E, OP> and k_series2i_compose<E, GLDS> run the same bodies on Interval<F64>
// (E = EIv, tests/series2_interval_isa_check.hip), every step through the functor: E::zero, add, neg, mul, mac, div, from_u32, exp,
// log, with mac / mulw / addw's wave-uniform shortcut (their ballot sees the active lanes only, so they stand inside the divergent
// loops).  In global memory an interval array is two planes (lo, hi) a plane stride apart; in LDS an interval is ONE 16-byte
// element {lo, hi} (S2Iv, the dynamic LDS declared 16-byte aligned): staging interleaves on the write, and the inner loops of mul
// and compose read one ds_read_b128 per operand.  All LDS sizes below are in elements: 8 bytes for EF64, 16 for EIv.
#pragma once
#include <hip/hip_runtime.h>

#include "gft_elem.hpp"
#include "gft_series.hpp"
#include "gft_series_kernels.hpp"  // rec_exp, rec_log: row 0 of exp / log is the univariate loop

namespace gft {

// ---- the LDS element of a functor -------------------------------------------------------------------------------------------------
struct alignas(16) S2Iv {  // an interval in LDS: one aligned 16-byte element
    double lo, hi;
};
template <class E>
struct S2L;
template <>
struct S2L<EF64> {
    typedef double T;
    __device__ static double get(const double* p, int i) { return p[i]; }
    __device__ static void put(double* p, unsigned i, double v) { p[i] = v; }
};
template <>
struct S2L<EIv> {
    typedef S2Iv T;
    __device__ static Iv get(const S2Iv* p, int i) {
        const S2Iv t = p[i];
        return Iv{t.lo, t.hi};
    }
    __device__ static void put(S2Iv* p, unsigned i, Iv v) { p[i] = S2Iv{v.lo, v.hi}; }
};
// a row of an LDS array as rec_exp / rec_log take it
template <class E>
struct S2Row {
    typename S2L<E>::T* p;
    __device__ typename E::V ld(unsigned i) const { return S2L<E>::get(p, (int)i); }
    __device__ void st(unsigned i, typename E::V v) const { S2L<E>::put(p, i, v); }
};
// the second factor of s2_mul_out: compact in LDS, or in global memory at its row stride (planes `plane` apart)
template <class E>
struct S2InLds {
    const typename S2L<E>::T* p;
    __device__ S2InLds at(size_t off) const { return S2InLds{p + off}; }
    __device__ typename E::V ld(int i) const { return S2L<E>::get(p, i); }
};
template <class E>
struct S2InGlobal {
    const double* p;
    size_t plane;
    __device__ S2InGlobal at(size_t off) const { return S2InGlobal{p + off, plane}; }
    __device__ typename E::V ld(int i) const {
        if constexpr (E::W == 1) return p[i];
        else return E::ld(p + i, plane, 0);
    }
};

// rows x cols elements from global rows `rstride` apart (planes `plane` apart) into a compact LDS array
template <class E>
__device__ inline void s2_stage(typename S2L<E>::T* lds, const double* src, size_t plane, size_t rstride, unsigned rows, unsigned cols) {
    const unsigned total = rows * cols;
    for (unsigned i = threadIdx.x; i < total; i += blockDim.x) {
        const unsigned r = i / cols, c = i - r * cols;
        S2L<E>::put(lds, i, E::ld(src, plane, (size_t)r * rstride + c));
    }
}
// the item's result from its compact LDS array: after a __syncthreads that follows every global load of this workgroup, so the
// result may be an operand itself
template <class E>
__device__ inline void s2_store(double* res, size_t plane, size_t rstride, const typename S2L<E>::T* lds, unsigned rows, unsigned cols) {
    const unsigned total = rows * cols;
    for (unsigned i = threadIdx.x; i < total; i += blockDim.x) {
        const unsigned r = i / cols, c = i - r * cols;
        E::st(res, plane, (size_t)r * rstride + c, S2L<E>::get(lds, (int)i));
    }
}

// ---- mul (mt:984-1012) ------------------------------------------------------------------------------------------------------
// z[k0][k1] = 0 + sum_{j0} (0 + sum_{j1} x[j0][j1] * y[k0-j0][k1-j1]), both ascending over the stored coefficients.
// x has pitch d.nx1; `yp` is the pitch of y: d.ny1 for a staged y, its row stride where it stays in global memory.
template <class E, class YA>
__device__ inline typename E::V s2_mul_out(const typename S2L<E>::T* xl, const YA yl, const Series2Dims& d, size_t yp, unsigned k0, unsigned k1) {
    typedef typename E::V V;
    const unsigned lo0 = k0 + 1 > d.ny0 ? k0 + 1 - d.ny0 : 0, hi0 = k0 + 1 < d.nx0 ? k0 + 1 : d.nx0;
    const unsigned lo1 = k1 + 1 > d.ny1 ? k1 + 1 - d.ny1 : 0, hi1 = k1 + 1 < d.nx1 ? k1 + 1 : d.nx1;
    V z = E::zero();
    for (unsigned j0 = lo0; j0 < hi0; ++j0) {
        const typename S2L<E>::T* xr = xl + j0 * d.nx1;
        const YA yr = yl.at((k0 - j0) * yp + k1);
        V o = E::zero();
#pragma unroll 4
        for (unsigned j1 = lo1; j1 < hi1; ++j1) o = E::mac(o, S2L<E>::get(xr, (int)j1), yr.ld(-(int)j1));
        z = E::addw(z, o);
    }
    return z;
}
// x and y staged compactly.  Thread t owns the outputs t and N - 1 - t of the row-major item, (k0, k1) and (n0-1-k0, n1-1-k1): a
// heavy output with a light one, as mul form B pairs k with n - 1 - k.  Lanes of a wave take consecutive k1, so the x address is
// wave-uniform where the bounds agree and the y addresses are consecutive.
template <class E>
__device__ inline void s2_mul_body(typename S2L<E>::T* lds, const double* x, const double* y, double* res, const Series2Dims& d,
                                   const SeriesBatch& g, const SeriesPlanes& pl) {
    typedef typename S2L<E>::T T;  // [nx0][nx1] | [ny0][ny1]
    T* xl = lds;
    T* yl = lds + d.nx0 * d.nx1;
    const SeriesOff o = series_offsets(g, blockIdx.x);
    s2_stage<E>(xl, x + o.x, pl.x, d.xr, d.nx0, d.nx1);
    s2_stage<E>(yl, y + o.y, pl.y, d.yr, d.ny0, d.ny1);
    __syncthreads();  // (every global load of this workgroup is done: the result may be x or y)
    const unsigned N = d.n0 * d.n1, half = (N + 1) / 2;
    for (unsigned t = threadIdx.x; t < half; t += blockDim.x) {
        const unsigned is[2] = {t, N - 1 - t};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned i = is[h];
            if (h == 1 && i == is[0]) break;  // the middle output of an odd N
            const unsigned k0 = i / d.n1, k1 = i - k0 * d.n1;
            E::st(res, pl.r, o.r + (size_t)k0 * d.rr + k1, s2_mul_out<E>(xl, S2InLds<E>{yl}, d, d.ny1, k0, k1));
        }
    }
}
#ifndef GFT_SERIES2_BODIES_ONLY  // (the one kernel here that is no template: gft_series3_kernels.hpp takes the bodies without it)
__global__ __launch_bounds__(256) void k_series2_mul(const double* x, const double* y, double* res, Series2Dims d, SeriesBatch g) {
    extern __shared__ double s2_lds[];
    s2_mul_body<EF64>(s2_lds, x, y, res, d, g, SeriesPlanes());
}
#endif
template <class E>
__global__ __launch_bounds__(256) void k_series2i_mul(const double* x, const double* y, double* res, Series2Dims d, SeriesBatch g, SeriesPlanes pl) {
    extern __shared__ S2Iv s2_lds_iv[];
    s2_mul_body<E>(s2_lds_iv, x, y, res, d, g, pl);
}

// ---- compose (subst_var's Horner path, mt:569-579) --------------------------------------------------------------------------------
// res = f(g) with g in the place of variable `var` of f.  The slices of f along that axis are its rows (var 0) or its columns (var 1);
// with S of them and `len` coefficients each:
//   res = 0.0 + slice S-1, stored shape (1, len) / (len, 1);  for i = S-2 .. 0:  res = mul(res, g) at the compact shape
//   L = (min(r0 + ng0 - 1, n0), min(r1 + ng1 - 1, n1)) of sum_shape;  row 0 / column 0 of res += slice i
// One workgroup runs the whole loop of its item (the steps are a dependency chain).  Two result arrays of n0 * n1 elements take turns
// in LDS, the current one compact at pitch r1; g sits compact behind them (GLDS) or stays in global memory at its row stride (the
// fallback where 2 N + ng0 * ng1 elements exceed the granted LDS).  Every step is k_series2_mul's pairing on a Series2Dims built for
// the step: a thread owns the outputs t and L0 * L1 - 1 - t, all bounds the same for every item; up to 512 lanes.  The owner of an output on the
// added slice loads f's coefficient before its sums and adds it after them -- with GLDS the only global traffic between steps,
// which meet through LDS alone.  f and g are read completely before the first store: the result may be f or g itself.
template <class E, bool GLDS>
__device__ inline void s2_compose_body(typename S2L<E>::T* lds, const double* f, const double* g, double* res, const Series2Dims& d, int var,
                                       const SeriesBatch& b, const SeriesPlanes& pl) {
    typedef typename E::V V;
    typedef typename S2L<E>::T T;  // res [n0 * n1] | res [n0 * n1] | (GLDS) g [ng0][ng1]
    const unsigned N = d.n0 * d.n1, tid = threadIdx.x, nt = blockDim.x;
    T* cur = lds;
    T* nxt = lds + N;
    T* gl = lds + 2 * N;
    const SeriesOff o = series_offsets(b, blockIdx.x);
    const double* fg = f + o.x;
    if (GLDS) s2_stage<E>(gl, g + o.y, pl.y, d.yr, d.ny0, d.ny1);
    const size_t gp = GLDS ? d.ny1 : d.yr;
    // slice i of f is fg[i * fslice + c * fstep], c < len
    const unsigned slices = var == 0 ? d.nx0 : d.nx1, len = var == 0 ? d.nx1 : d.nx0;
    const size_t fslice = var == 0 ? d.xr : 1, fstep = var == 0 ? 1 : d.xr;
    for (unsigned c = tid; c < len; c += nt) S2L<E>::put(cur, c, E::add(E::zero(), E::ld(fg, pl.x, (slices - 1) * fslice + c * fstep)));
    __syncthreads();
    unsigned r0 = var == 0 ? 1 : len, r1 = var == 0 ? len : 1;  // the stored shape of res
    for (unsigned i = slices - 1; i-- > 0;) {
        Series2Dims s;
        s.nx0 = r0, s.nx1 = r1, s.ny0 = d.ny0, s.ny1 = d.ny1;
        s.n0 = r0 + d.ny0 - 1 < d.n0 ? r0 + d.ny0 - 1 : d.n0;
        s.n1 = r1 + d.ny1 - 1 < d.n1 ? r1 + d.ny1 - 1 : d.n1;
        const unsigned M = s.n0 * s.n1, half = (M + 1) / 2;
        const double* fi = fg + i * fslice;
        for (unsigned t = tid; t < half; t += nt) {
            const unsigned is[2] = {t, M - 1 - t};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned idx = is[h];
                if (h == 1 && idx == is[0]) break;  // the middle output of an odd M
                const unsigned k0 = idx / s.n1, k1 = idx - k0 * s.n1;
                const bool added = var == 0 ? (k0 == 0 && k1 < len) : (k1 == 0 && k0 < len);
                V fv = E::zero();
                if (added) fv = E::ld(fi, pl.x, (var == 0 ? k1 : k0) * fstep);  // in flight during the sums below
                V z;
                if (GLDS) z = s2_mul_out<E>(cur, S2InLds<E>{gl}, s, gp, k0, k1);
                else z = s2_mul_out<E>(cur, S2InGlobal<E>{g + o.y, pl.y}, s, gp, k0, k1);
                if (added) z = E::add(z, fv);
                S2L<E>::put(nxt, idx, z);
            }
        }
        lds_barrier();
        T* sw = cur;
        cur = nxt;
        nxt = sw;
        r0 = s.n0, r1 = s.n1;
    }
    __syncthreads();  // (every global load of this workgroup is done: the result may be f or g)
    for (unsigned idx = tid; idx < N; idx += nt) {
        const unsigned k0 = idx / d.n1, k1 = idx - k0 * d.n1;
        E::st(res, pl.r, o.r + (size_t)k0 * d.rr + k1, k0 < r0 && k1 < r1 ? S2L<E>::get(cur, (int)(k0 * r1 + k1)) : E::zero());
    }
}
template <bool GLDS>
__global__ __launch_bounds__(512) void k_series2_compose(const double* f, const double* g, double* res, Series2Dims d, int var, SeriesBatch b) {
    extern __shared__ double s2_lds[];
    s2_compose_body<EF64, GLDS>(s2_lds, f, g, res, d, var, b, SeriesPlanes());
}
template <class E, bool GLDS>
__global__ __launch_bounds__(512) void k_series2i_compose(const double* f, const double* g, double* res, Series2Dims d, int var, SeriesBatch b,
                                                          SeriesPlanes pl) {
    extern __shared__ S2Iv s2_lds_iv[];
    s2_compose_body<E, GLDS>(s2_lds_iv, f, g, res, d, var, b, pl);
}

// ---- corr, the transposed product (the adjoint of mul; F64 only) -------------------------------------------------------------------
// c[i0][i1] = 0 + sum_{k0} (0 + sum_{k1} g[k0][k1] * y[k0-i0][k1-i1]), both DESCENDING over the stored coefficients: k0 from
// min(g0-1, i0+ny0-1) to i0, k1 from min(g1-1, i1+ny1-1) to i1.  With j = g-1-k ascending these are the sums of s2_mul_out on the
// array flipped along both axes: c[i0][i1] is bit for bit mul(flip(g), y, (g0, g1))[g0-1-i0][g1-1-i1].  So g is staged FLIPPED
// (element i of the row-major item at g0 * g1 - 1 - i) and an output is s2_mul_out itself, the same inner loops as mul.
template <class E>
__device__ inline void s2_stage_flipped(typename S2L<E>::T* lds, const double* src, size_t rstride, unsigned rows, unsigned cols) {
    const unsigned total = rows * cols;
    for (unsigned i = threadIdx.x; i < total; i += blockDim.x) {
        const unsigned r = i / cols, c = i - r * cols;
        S2L<E>::put(lds, total - 1 - i, E::ld(src, 0, (size_t)r * rstride + c));
    }
}
// The outputs of one step from `fl` = flip(a), a of stored shape (g0, g1): thread t owns the outputs M - 1 - t and t of the
// row-major (m0, m1) result, in that order -- the light one first, as s2_mul_body runs its pair (here the heavy outputs are the LOW
// indices: output (0, 0) has every term, the last one a single product).  With m == g this is mul's assignment of outputs to lanes
// exactly.  fn(idx, i0, i1, sum) stores.
template <class E, class YA, class F>
__device__ inline void s2_corr_pairs(const typename S2L<E>::T* fl, unsigned g0, unsigned g1, const YA yl, unsigned ny0, unsigned ny1, size_t yp,
                                     unsigned m0, unsigned m1, F fn) {
    Series2Dims s;  // of the product flip(a) * y (s2_mul_out reads the operands' shapes only)
    s.nx0 = g0, s.nx1 = g1, s.ny0 = ny0, s.ny1 = ny1;
    const unsigned M = m0 * m1, half = (M + 1) / 2;
    for (unsigned t = threadIdx.x; t < half; t += blockDim.x) {
        const unsigned is[2] = {M - 1 - t, t};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned idx = is[h];
            if (h == 1 && idx == is[0]) break;  // the middle output of an odd M
            const unsigned i0 = idx / m1, i1 = idx - i0 * m1;
            fn(idx, i0, i1, s2_mul_out<E>(fl, yl, s, yp, g0 - 1 - i0, g1 - 1 - i1));
        }
    }
}
// d: x is g (nx0, nx1), y is y (ny0, ny1) <= g, the result (n0, n1) <= g.  g and y staged compactly, every global load before the
// first store: the result may be g itself (the same view); the host refuses a result that overlaps y.
template <class E>
__global__ __launch_bounds__(256) void k_series2_corr(const double* g, const double* y, double* res, Series2Dims d, SeriesBatch b) {
    extern __shared__ double s2_lds[];  // flip(g) [g0][g1] | [ny0][ny1]
    double* gl = s2_lds;
    double* yl = s2_lds + d.nx0 * d.nx1;
    const SeriesOff o = series_offsets(b, blockIdx.x);
    s2_stage_flipped<E>(gl, g + o.x, d.xr, d.nx0, d.nx1);
    s2_stage<E>(yl, y + o.y, 0, d.yr, d.ny0, d.ny1);
    __syncthreads();  // (every global load of this workgroup is done: the result may be g)
    s2_corr_pairs<E>(gl, d.nx0, d.nx1, S2InLds<E>{yl}, d.ny0, d.ny1, d.ny1, d.n0, d.n1,
                     [&](unsigned, unsigned i0, unsigned i1, typename E::V sum) { E::st(res, 0, o.r + (size_t)i0 * d.rr + i1, sum); });
}

// ---- compose_adj, the transposed Horner loop (the gradient of compose with respect to f; F64 only) ------------------------------
// d: x is gh (nx0, nx1) = the n of the composition, y is g (ny0, ny1) <= n, the result f's stored shape (n0, n1) <= n.  With S slices
// of f of `len` coefficients (rows for var 0, columns for var 1) and base = (1, len) / (len, 1), the forward loop's compact shapes
// are L_i = min(base + (S-1-i) * (ng - 1), n) per axis.  a_0 = gh[:L_0]; slice i of the result is the first `len` entries of row 0
// / column 0 of a_i; a_{i+1} = corr(a_i, g) at the result shape L_{i+1} (s2_corr_pairs at the compact shapes).  The mirror of
// s2_compose_body: one workgroup runs the whole loop of its item, two arrays of n0 * n1 elements take turns in LDS, the current one
// compact at pitch L_i[1] and FLIPPED, as corr wants its first operand; g sits compact behind them (GLDS) or stays in global memory
// at its row stride.  The owner of an output on row 0 / column 0 stores it to the result as well, so the steps meet through LDS
// alone.  gh is read completely before the first store: the result may be gh itself (the same view); it never overlaps g (the host
// refuses that).
template <class E, bool GLDS>
__global__ __launch_bounds__(512) void k_series2_compose_adj(const double* gh, const double* g, double* res, Series2Dims d, int var, SeriesBatch b) {
    extern __shared__ double s2_lds[];  // flip(a) [nx0 * nx1] | flip(a) [nx0 * nx1] | (GLDS) g [ng0][ng1]
    const unsigned N = d.nx0 * d.nx1, tid = threadIdx.x, nt = blockDim.x;
    double* cur = s2_lds;
    double* nxt = s2_lds + N;
    double* gl = s2_lds + 2 * N;
    const SeriesOff o = series_offsets(b, blockIdx.x);
    double* rg = res + o.r;
    const unsigned slices = var == 0 ? d.n0 : d.n1, len = var == 0 ? d.n1 : d.n0;
    const size_t rslice = var == 0 ? d.rr : 1, rstep = var == 0 ? 1 : d.rr;  // slice i of the result is rg[i * rslice + c * rstep], c < len
    const unsigned b0 = var == 0 ? 1 : len, b1 = var == 0 ? len : 1;
    auto shape = [&](unsigned i, unsigned& l0, unsigned& l1) {  // L_i
        const unsigned k = slices - 1 - i, f0 = b0 + k * (d.ny0 - 1), f1 = b1 + k * (d.ny1 - 1);
        l0 = f0 < d.nx0 ? f0 : d.nx0;
        l1 = f1 < d.nx1 ? f1 : d.nx1;
    };
    unsigned r0, r1;  // the stored shape of a
    shape(0, r0, r1);
    if (GLDS && slices > 1) s2_stage<E>(gl, g + o.y, 0, d.yr, d.ny0, d.ny1);
    s2_stage_flipped<E>(cur, gh + o.x, d.xr, r0, r1);
    __syncthreads();  // (every global load of gh is done: the result may be gh)
    for (unsigned c = tid; c < len; c += nt) rg[c * rstep] = cur[r0 * r1 - 1 - (var == 0 ? c : c * r1)];  // a_0[0][c] / a_0[c][0]
    const size_t gp = GLDS ? d.ny1 : d.yr;
    for (unsigned i = 1; i < slices; ++i) {
        unsigned m0, m1;
        shape(i, m0, m1);
        double* ri = rg + i * rslice;
        const unsigned last = m0 * m1 - 1;
        auto put = [&](unsigned idx, unsigned i0, unsigned i1, double sum) {
            nxt[last - idx] = sum;
            if (var == 0 ? (i0 == 0 && i1 < len) : (i1 == 0 && i0 < len)) ri[(var == 0 ? i1 : i0) * rstep] = sum;
        };
        if (GLDS) s2_corr_pairs<E>(cur, r0, r1, S2InLds<E>{gl}, d.ny0, d.ny1, gp, m0, m1, put);
        else s2_corr_pairs<E>(cur, r0, r1, S2InGlobal<E>{g + o.y, 0}, d.ny0, d.ny1, gp, m0, m1, put);
        lds_barrier();
        double* sw = cur;
        cur = nxt;
        nxt = sw;
        r0 = m0, r1 = m1;
    }
}

// ---- the 1-d division of a row in place (mt:1162-1192 at one axis: rec_div with a full-length dividend) -----------------------
// row[i] = (-(0 + sum_{j = lo .. i-1} row[j] * yv[i-j]) + row[i]) / yv[0], lo = max(0, i + 1 - ny1).  Lane i's sum needs row[j] at
// its j-th step and row[j] is final after j steps, so the P participating lanes advance in lock step over j (the schedule of
// div_1d_body, gft_div2d.hip, on a row that already sits in LDS): the owner of j finalises and publishes it, everybody adds its
// term.  WAVE: the participants are one wave, which orders its own LDS traffic without a workgroup barrier.
template <bool WAVE>
__device__ inline void s2_step_sync() {
    if (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    } else {
        lds_barrier();
    }
}
constexpr unsigned S2_WAVE_EPT = 8;    // rows up to 512 coefficients: one wave, 8 coefficients a lane
constexpr unsigned S2_BLOCK_EPT = 16;  // longer rows (then the workgroup has 256 lanes): 16 a lane, 4096 at most
constexpr unsigned S2_BLOCK_EPT_IV = 8;  // intervals: rows of 2048 at most, and an accumulator is two register pairs
template <class E, bool WAVE>
__device__ __forceinline__ void s2_div1d(typename S2L<E>::T* row, const typename S2L<E>::T* yv, unsigned ny1, unsigned n1, unsigned tid, unsigned P) {
    typedef typename E::V V;
    constexpr unsigned EPT = WAVE ? S2_WAVE_EPT : (E::W == 2 ? S2_BLOCK_EPT_IV : S2_BLOCK_EPT);
    V cur[EPT];
#pragma unroll
    for (unsigned e = 0; e < EPT; ++e) cur[e] = E::zero();
    const V y0 = S2L<E>::get(yv, 0);
    for (unsigned j = 0; j < n1; ++j) {
        const unsigned oe = j / P;
        if (tid == j - oe * P) {
#pragma unroll
            for (unsigned e = 0; e < EPT; ++e)
                if (e == oe) S2L<E>::put(row, j, E::div(E::add(E::neg(cur[e]), S2L<E>::get(row, (int)j)), y0));
        }
        s2_step_sync<WAVE>();
        const V q = S2L<E>::get(row, (int)j);
#pragma unroll
        for (unsigned e = 0; e < EPT; ++e) {
            const unsigned i = tid + e * P;
            if (i < n1 && i > j && i - j < ny1) cur[e] = E::mac(cur[e], q, S2L<E>::get(yv, (int)(i - j)));
        }
    }
}

// ---- div (mt:1162-1192), exp (mt:1285-1317), log (mt:1335-1386) -------------------------------------------------------------------
// A is the operand resident beside the result r: div's y, exp's and log's x.  div reads its dividend row x[k] from global memory
// in the step of row k; the result is stored once at the end, so it may be x (or y) itself.
//   div  c = sum_{j = max(0,k+1-ny0) .. k-1} mul_1d(r[j], y[k-j]);  c = -c;  c[:nx1] += x[k] (k < nx0);  r[k] = div_1d(c, y[0])
//   exp  r[0] = exp_1d(x[0]);  c = sum_{j = 1 .. min(nx0,k+1)-1} mul_1d(x[j] * j, r[k-j]);  r[k] = c / k
//   log  r[0] = log_1d(x[0]);  c = sum_{j = max(1,k+1-nx0) .. k-1} mul_1d(x[k-j], r[j] * j);  c = -c;  c[:nx1] += k * x[k] (k < nx0);
//        r[k] = div_1d(c, x[0]) / k
// `y`: div's divisor; exp / log: the seeds exp(x[0][0]) / ln(x[0][0]) per item, or null (formed here by the device library).
// j and k enter as E::from_u32 (the reference's S::from_u32): with intervals the point [j, j], whose product with a coefficient is
// the functor's mul, short-circuits included ([1,1] * b is b).
// The rows of one item on arrays that sit in LDS: A [a0][a1] | r [n0][n1] | `sl`: scratch of `srows` rows of n1.  `xg`: div's
// dividend, the item's x in global memory (rows `xr` and coefficients `xc` apart -- 1 at rank 2 --, planes `xplane`); `seed`: the item's seed of exp / log, or null.
// LDSDIV (div only): the dividend is r itself, all n0 x n1 of it, divided in place -- the slab step of rank 3
// (gft_series3_kernels.hpp).  Row k of it is read in the step of row k, so the accumulator of that row lives in the first n1
// elements of `sl` between the chunks and the row sums behind them: `sl` then holds n1 + srows * n1 elements.
template <class E, int OP, bool LDSDIV = false>
__device__ inline void s2_rec_rows(const typename S2L<E>::T* al, unsigned a0, unsigned a1, typename S2L<E>::T* rl, unsigned n0, unsigned n1,
                                   typename S2L<E>::T* sl, unsigned srows, const double* xg, size_t xplane, size_t xr, size_t xc, unsigned nx0, unsigned nx1,
                                   const double* seed, size_t splane) {
    typedef typename E::V V;
    typedef typename S2L<E>::T T;
    constexpr bool DIV = OP == SERIES_DIV, EXP = OP == SERIES_EXP;
    static_assert(DIV || !LDSDIV, "only div takes its dividend from LDS");
    const unsigned tid = threadIdx.x, nt = blockDim.x;
    if (LDSDIV) sl += n1;
    if (!DIV) {  // row 0: the univariate recurrence, a dependency chain on one lane
        if (tid == 0) {
            const S2Row<E> xr0{const_cast<T*>(al)}, rr{rl};
            const V sd = seed ? E::ld(seed, splane, 0) : (EXP ? E::exp(S2L<E>::get(al, 0)) : E::log(S2L<E>::get(al, 0)));
            if (EXP) rec_exp<E>(xr0, rr, a1, n1, sd);
            else rec_log<E>(xr0, rr, a1, n1, sd);
        }
        lds_barrier();
    }
    for (unsigned k = DIV ? 0u : 1u; k < n0; ++k) {
        unsigned jlo, jhi;  // the terms of row k, ascending
        if (EXP) {
            jlo = 1;
            jhi = a0 < k + 1 ? a0 : k + 1;
        } else {
            jlo = k + 1 > a0 ? k + 1 - a0 : 0;
            if (!DIV && jlo < 1) jlo = 1;
            jhi = k;
        }
        T* rk = rl + k * n1;
        T* ck = LDSDIV ? sl - n1 : rk;  // the accumulator of row k between the chunks
        for (unsigned jb = jlo; jb < jhi; jb += srows) {
            const unsigned cnt = jhi - jb < srows ? jhi - jb : srows;
            // pass 1: the row sums of the chunk, one (j, k1) a lane
            for (unsigned idx = tid; idx < cnt * n1; idx += nt) {
                const unsigned jj = idx / n1, k1 = idx - jj * n1, j = jb + jj;
                V s = E::zero();
                if (DIV) {  // mul_1d(r[j], y[k-j]): r[j] has n1 coefficients, y[k-j] has ny1
                    const T* a = rl + j * n1;
                    const T* b = al + (k - j) * a1 + k1;
                    const unsigned lo = k1 + 1 > a1 ? k1 + 1 - a1 : 0;
#pragma unroll 4
                    for (unsigned j1 = lo; j1 <= k1; ++j1) s = E::mac(s, S2L<E>::get(a, (int)j1), S2L<E>::get(b, -(int)j1));
                } else {
                    const V fj = E::from_u32(j);
                    const unsigned hi = k1 + 1 < a1 ? k1 + 1 : a1;
                    if (EXP) {  // mul_1d(x[j] * j, r[k-j]): x[j] * j is rounded before it meets r
                        const T* a = al + j * a1;
                        const T* b = rl + (k - j) * n1 + k1;
#pragma unroll 4
                        for (unsigned j1 = 0; j1 < hi; ++j1) s = E::mac(s, E::mulw(S2L<E>::get(a, (int)j1), fj), S2L<E>::get(b, -(int)j1));
                    } else {  // mul_1d(x[k-j], r[j] * j)
                        const T* a = al + (k - j) * a1;
                        const T* b = rl + j * n1 + k1;
#pragma unroll 4
                        for (unsigned j1 = 0; j1 < hi; ++j1) s = E::mac(s, S2L<E>::get(a, (int)j1), E::mulw(S2L<E>::get(b, -(int)j1), fj));
                    }
                }
                S2L<E>::put(sl, idx, s);
            }
            lds_barrier();
            // pass 2: the ordered additions; r[k] (LDSDIV: the head of the scratch) carries the accumulator from chunk to chunk
            for (unsigned k1 = tid; k1 < n1; k1 += nt) {
                V c = jb == jlo ? E::zero() : S2L<E>::get(ck, (int)k1);
                for (unsigned jj = 0; jj < cnt; ++jj) c = E::addw(c, S2L<E>::get(sl, (int)(jj * n1 + k1)));
                S2L<E>::put(ck, k1, c);
            }
            lds_barrier();
        }
        // the row's own step (a lane meets the k1 it owned in pass 2)
        for (unsigned k1 = tid; k1 < n1; k1 += nt) {
            V c = jlo < jhi ? S2L<E>::get(ck, (int)k1) : E::zero();
            if (EXP) {
                c = E::div(c, E::from_u32(k));
            } else {
                c = E::neg(c);
                if (LDSDIV) c = E::add(c, S2L<E>::get(rk, (int)k1));
                else if (k < nx0 && k1 < nx1)
                    c = E::add(c, DIV ? E::ld(xg, xplane, (size_t)k * xr + k1 * xc) : E::mul(E::from_u32(k), S2L<E>::get(al, (int)(k * a1 + k1))));
            }
            S2L<E>::put(rk, k1, c);
        }
        lds_barrier();
        if (!EXP) {
            if (n1 <= 64 * S2_WAVE_EPT) {
                if (tid < 64) s2_div1d<E, true>(rk, al, a1, n1, tid, 64);
            } else {
                s2_div1d<E, false>(rk, al, a1, n1, tid, nt);
            }
            lds_barrier();
            if (!DIV) {
                for (unsigned k1 = tid; k1 < n1; k1 += nt) S2L<E>::put(rk, k1, E::div(S2L<E>::get(rk, (int)k1), E::from_u32(k)));
                lds_barrier();
            }
        }
    }
}
template <class E, int OP>
__device__ inline void s2_rec_body(typename S2L<E>::T* lds, const double* x, const double* y, double* res, const Series2Dims& d, unsigned srows,
                                   const SeriesBatch& g, const SeriesPlanes& pl) {
    typedef typename S2L<E>::T T;  // A [a0][a1] | r [n0][n1] | scratch [srows][n1]
    constexpr bool DIV = OP == SERIES_DIV;
    const unsigned a0 = DIV ? d.ny0 : d.nx0, a1 = DIV ? d.ny1 : d.nx1, n1 = d.n1;
    T* al = lds;
    T* rl = al + a0 * a1;
    T* sl = rl + d.n0 * n1;
    const SeriesOff o = series_offsets(g, blockIdx.x);
    if (DIV) s2_stage<E>(al, y + o.y, pl.y, d.yr, a0, a1);
    else s2_stage<E>(al, x + o.x, pl.x, d.xr, a0, a1);
    __syncthreads();
    s2_rec_rows<E, OP>(al, a0, a1, rl, d.n0, n1, sl, srows, x + o.x, pl.x, d.xr, 1, d.nx0, d.nx1, !DIV && y ? y + o.s : nullptr, pl.s);
    __syncthreads();  // (every global load of this workgroup is done: the result may be an operand)
    s2_store<E>(res + o.r, pl.r, d.rr, rl, d.n0, n1);
}
template <int OP>
__global__ __launch_bounds__(256) void k_series2_rec(const double* x, const double* y, double* res, Series2Dims d, unsigned srows,
                                                     SeriesBatch g) {
    extern __shared__ double s2_lds[];
    s2_rec_body<EF64, OP>(s2_lds, x, y, res, d, srows, g, SeriesPlanes());
}
template <class E, int OP>
__global__ __launch_bounds__(256) void k_series2i_rec(const double* x, const double* y, double* res, Series2Dims d, unsigned srows, SeriesBatch g,
                                                      SeriesPlanes pl) {
    extern __shared__ S2Iv s2_lds_iv[];
    s2_rec_body<E, OP>(s2_lds_iv, x, y, res, d, srows, g, pl);
}

}  // namespace gft
