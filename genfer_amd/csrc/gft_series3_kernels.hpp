// Device side of the batched trivariate series (gft_series3.hip plans and launches these).  One workgroup is one item for the
// whole operation, the operands resident in LDS, as at rank 2 (gft_series2_kernels.hpp, whose bodies this file builds on).
//
// An item is an [n0, n1, n2] coefficient array in the PERMUTED order of Series3Dims (gft_series_args.hpp): the unit axes of the
// stored result shape S in front, so every axis has its own element stride in global memory and LDS holds the arrays compactly
// in that order.  Axis 0 are the slabs, axis 1 the rows of a slab.  Every operation is the reference's recursion over axis 0
// (mul mt:984-1012, div mt:1162-1192, exp mt:1285-1317, log mt:1335-1386) whose terms are the univariate products
// mul_1d(a, b)[k2] = 0.0 + sum_{j2} a[j2] * b[k2 - j2] of two rows, added for j0 ascending and inside it j1 ascending to the ONE
// accumulator of row (k0, k1): "independent row sums, ordered additions".
//   mul            a thread owns whole outputs (k0, k1, k2) and runs the three sums; no step depends on another.
//   compose        the Horner chain of such products, the result resident in LDS from step to step (k_series3_compose).
//   div, exp, log  slabs k0 one after the other.  The terms of output row k1 are the pairs (j0, j1), numbered t = j0' * J1 + j1'
//                  with J1 = min(n1, a1) places for j1 of which row k1 uses the first min(k1 + 1, a1).  Pass 1 forms the row sums
//                  of a chunk of t for every k1 in parallel over (t, k1, k2) into the LDS scratch, pass 2 adds them in ascending
//                  t into r[k0] (which holds the accumulators between chunks); then the slab's own step: negate and add the
//                  dividend, the RANK-2 division by slab 0 of the divisor on the slab where it sits (s2_rec_rows with its
//                  dividend in LDS), the division by k0.  Slab 0 of exp / log is the rank-2 body s2_rec_rows on slab 0 of x.
//                  Chunking changes how many row sums are in flight, never the order of an addition.
// With n0 == 1 these ARE the rank-2 loops (one slab, no terms), with n0 == n1 == 1 the rank-1 loops: how an S with unit axes
// is computed.  Multiply and add are rounded separately (-ffp-contract=off) and no explicit fma is written.
// The bodies are templates over the element functor (gft_elem.hpp) as at rank 2.  k_series3_mul, k_series3_rec<OP> and
// k_series3_compose<GLDS> are the EF64 kernels; k_series3i_mul<E>, k_series3i_rec<E, OP> and k_series3i_compose<E, GLDS> run the same
// bodies on Interval<F64> (E = EIv, emitted where gft_series3.hip instantiates them): two planes a plane stride apart in global
// memory, ONE 16-byte element {lo, hi} in LDS (S2Iv), so every LDS size below is in elements of 8 (EF64) or 16 bytes (EIv).
// Every barrier stands under loops whose trip counts come from the shapes in Series3Dims and the plan, the same for every lane.
#pragma once
#include <hip/hip_runtime.h>

#define GFT_SERIES2_BODIES_ONLY  // k_series2_mul is defined where gft_series2.hip includes that header
#include "gft_series2_kernels.hpp"

namespace gft {

// d0 x d1 x d2 elements from global memory at the strides st[] (planes `plane` apart) into a compact LDS array
template <class E>
__device__ inline void s3_stage(typename S2L<E>::T* lds, const double* src, size_t plane, const size_t* st, const unsigned* dims) {
    const unsigned d12 = dims[1] * dims[2], total = dims[0] * d12;
    for (unsigned i = threadIdx.x; i < total; i += blockDim.x) {
        const unsigned j0 = i / d12, r = i - j0 * d12, j1 = r / dims[2], j2 = r - j1 * dims[2];
        S2L<E>::put(lds, i, E::ld(src, plane, (size_t)j0 * st[0] + (size_t)j1 * st[1] + (size_t)j2 * st[2]));
    }
}
// everything of the caller's n outside S is +0.0 (in the caller's axis order)
template <class E, class D>
__device__ inline void s3_zero_fill(double* res, size_t plane, const D& d) {
    if (d.full[0] == d.keep[0] && d.full[1] == d.keep[1] && d.full[2] == d.keep[2]) return;
    const unsigned f12 = d.full[1] * d.full[2], total = d.full[0] * f12;
    for (unsigned i = threadIdx.x; i < total; i += blockDim.x) {
        const unsigned k0 = i / f12, r = i - k0 * f12, k1 = r / d.full[2], k2 = r - k1 * d.full[2];
        if (k0 >= d.keep[0] || k1 >= d.keep[1] || k2 >= d.keep[2])
            E::st(res, plane, (size_t)k0 * d.fs[0] + (size_t)k1 * d.fs[1] + (size_t)k2 * d.fs[2], E::zero());
    }
}

// ---- mul ----------------------------------------------------------------------------------------------------------------------
// z[k0][k1][k2] = 0 + sum_{j0} sum_{j1} (0 + sum_{j2} x[j0][j1][j2] * y[k0-j0][k1-j1][k2-j2]), all ascending over the stored
// coefficients, the row sum formed first and then added.  x and y staged compactly.  Thread t owns the outputs t and N - 1 - t of
// the row-major item: a heavy output with a light one, as s2_mul_body pairs them.  Lanes of a wave take consecutive k2.
// The second factor of s3_mul_out, as S2InLds / S2InGlobal at rank 2: compact in LDS at the pitches of its stored shape, or in global
// memory at the element strides of its three (permuted) axes -- the innermost one too, which is the row or the slab stride where S has
// unit axes.  row(i0, i1, k2) is the place of y[i0][i1][k2]; ld(-j2) then reads y[i0][i1][k2 - j2].
template <class E>
struct S3InLds {
    const typename S2L<E>::T* p;
    unsigned p0, p1;  // elements from slab to slab and from row to row
    __device__ S3InLds row(unsigned i0, unsigned i1, unsigned k2) const { return S3InLds{p + (i0 * p0 + i1 * p1) + k2, p0, p1}; }
    __device__ typename E::V ld(int i) const { return S2L<E>::get(p, i); }
};
template <class E>
struct S3InGlobal {
    const double* p;
    size_t plane, s0, s1, s2;
    __device__ S3InGlobal row(unsigned i0, unsigned i1, unsigned k2) const {
        return S3InGlobal{p + ((size_t)i0 * s0 + (size_t)i1 * s1 + (size_t)k2 * s2), plane, s0, s1, s2};
    }
    __device__ typename E::V ld(int i) const { return E::ld(p + (ptrdiff_t)i * (ptrdiff_t)s2, plane, 0); }
};
template <class E, class YA>
__device__ inline typename E::V s3_mul_out(const typename S2L<E>::T* xl, const YA yl, const Series3Dims& d, unsigned k0, unsigned k1, unsigned k2) {
    typedef typename E::V V;
    const unsigned lo0 = k0 + 1 > d.ny[0] ? k0 + 1 - d.ny[0] : 0, hi0 = k0 + 1 < d.nx[0] ? k0 + 1 : d.nx[0];
    const unsigned lo1 = k1 + 1 > d.ny[1] ? k1 + 1 - d.ny[1] : 0, hi1 = k1 + 1 < d.nx[1] ? k1 + 1 : d.nx[1];
    const unsigned lo2 = k2 + 1 > d.ny[2] ? k2 + 1 - d.ny[2] : 0, hi2 = k2 + 1 < d.nx[2] ? k2 + 1 : d.nx[2];
    V z = E::zero();
    for (unsigned j0 = lo0; j0 < hi0; ++j0)
        for (unsigned j1 = lo1; j1 < hi1; ++j1) {
            const typename S2L<E>::T* xr = xl + (j0 * d.nx[1] + j1) * d.nx[2];
            const YA yr = yl.row(k0 - j0, k1 - j1, k2);
            V o = E::zero();
#pragma unroll 4
            for (unsigned j2 = lo2; j2 < hi2; ++j2) o = E::mac(o, S2L<E>::get(xr, (int)j2), yr.ld(-(int)j2));
            z = E::addw(z, o);
        }
    return z;
}
template <class E>
__device__ inline void s3_mul_body(typename S2L<E>::T* lds, const double* x, const double* y, double* res, const Series3Dims& d, const SeriesBatch& g,
                                   const SeriesPlanes& pl) {
    typedef typename S2L<E>::T T;  // [nx0][nx1][nx2] | [ny0][ny1][ny2]
    T* xl = lds;
    T* yl = lds + d.nx[0] * d.nx[1] * d.nx[2];
    const SeriesOff o = series_offsets(g, blockIdx.x);
    s3_stage<E>(xl, x + o.x, pl.x, d.xs, d.nx);
    s3_stage<E>(yl, y + o.y, pl.y, d.ys, d.ny);
    __syncthreads();  // (every global load of this workgroup is done: the result may be x or y)
    const unsigned n12 = d.n[1] * d.n[2], N = d.n[0] * n12, half = (N + 1) / 2;
    for (unsigned t = threadIdx.x; t < half; t += blockDim.x) {
        const unsigned is[2] = {t, N - 1 - t};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned i = is[h];
            if (h == 1 && i == is[0]) break;  // the middle output of an odd N
            const unsigned k0 = i / n12, r = i - k0 * n12, k1 = r / d.n[2], k2 = r - k1 * d.n[2];
            E::st(res, pl.r, o.r + (size_t)k0 * d.rs[0] + (size_t)k1 * d.rs[1] + (size_t)k2 * d.rs[2], s3_mul_out<E>(xl, S3InLds<E>{yl, d.ny[1] * d.ny[2], d.ny[2]}, d, k0, k1, k2));
        }
    }
    s3_zero_fill<E>(res + o.r, pl.r, d);
}
__global__ __launch_bounds__(256) void k_series3_mul(const double* x, const double* y, double* res, Series3Dims d, SeriesBatch g) {
    extern __shared__ double s3_lds[];
    s3_mul_body<EF64>(s3_lds, x, y, res, d, g, SeriesPlanes());
}
template <class E>
__global__ __launch_bounds__(256) void k_series3i_mul(const double* x, const double* y, double* res, Series3Dims d, SeriesBatch g, SeriesPlanes pl) {
    extern __shared__ S2Iv s3_lds_iv[];
    s3_mul_body<E>(s3_lds_iv, x, y, res, d, g, pl);
}

// ---- compose (subst_var's Horner path, mt:569-579) ------------------------------------------------------------------------------
// res = f(g) with g in the place of one variable of f, on the PERMUTED item of Series3Compose (gft_series_args.hpp: the unit axes of
// the final stored shape S in front, the same for every step).  With `slices` slices of f along that variable's axis, each of the
// stored shape sl (f's with 1 on the axis):
//   res = 0.0 + the last slice, stored shape sl;  for i = slices-2 .. 0:  res = mul3(res, g) at the compact shape
//   L = min(r + ng - 1, n) per axis;  res[index 0 on the axis][inside sl] += slice i
// s2_compose_body with a slab axis: one workgroup runs the whole chain of its item.  Two result arrays of n0 * n1 * n2 elements take
// turns in LDS, the current one compact at its own pitches; g sits compact behind them (GLDS) or stays in global memory at its three
// strides (where 2 N + |g| elements exceed the granted LDS).  Every step is k_series3_mul's pairing on a Series3Dims built for the
// step: a thread owns the outputs t and M - 1 - t, all bounds the same for every item.  The owner of an output on the added slice
// loads f's coefficient before its sums and adds it after them.  f and g are read completely before the first store: the result
// may be f or g itself.
template <class E, bool GLDS>
__device__ inline void s3_compose_body(typename S2L<E>::T* lds, const double* f, const double* g, double* res, const Series3Compose& c,
                                       const SeriesBatch& b, const SeriesPlanes& pl) {
    typedef typename E::V V;
    typedef typename S2L<E>::T T;  // res [N] | res [N] | (GLDS) g [ng0][ng1][ng2]
    const unsigned N = c.full[0] * c.full[1] * c.full[2], tid = threadIdx.x, nt = blockDim.x;
    T* cur = lds;
    T* nxt = lds + N;
    T* gl = lds + 2 * N;
    const SeriesOff o = series_offsets(b, blockIdx.x);
    const double* fg = f + o.x;
    if (GLDS) s3_stage<E>(gl, g + o.y, pl.y, c.ys, c.ng);
    // the stored shape of res: it starts as a slice (1 on the substituted axis, so `inside sl` implies index 0 there)
    unsigned r0 = c.sl[0], r1 = c.sl[1], r2 = c.sl[2];
    {
        const double* fl = fg + (size_t)(c.slices - 1) * c.fslice;
        const unsigned r12 = r1 * r2, total = r0 * r12;
        for (unsigned i = tid; i < total; i += nt) {
            const unsigned k0 = i / r12, q = i - k0 * r12, k1 = q / r2, k2 = q - k1 * r2;
            S2L<E>::put(cur, i, E::add(E::zero(), E::ld(fl, pl.x, (size_t)k0 * c.xs[0] + (size_t)k1 * c.xs[1] + (size_t)k2 * c.xs[2])));
        }
    }
    __syncthreads();
    for (unsigned i = c.slices - 1; i-- > 0;) {
        Series3Dims s;
        s.nx[0] = r0, s.nx[1] = r1, s.nx[2] = r2;
        s.ny[0] = c.ng[0], s.ny[1] = c.ng[1], s.ny[2] = c.ng[2];
        s.n[0] = r0 + c.ng[0] - 1 < c.n[0] ? r0 + c.ng[0] - 1 : c.n[0];
        s.n[1] = r1 + c.ng[1] - 1 < c.n[1] ? r1 + c.ng[1] - 1 : c.n[1];
        s.n[2] = r2 + c.ng[2] - 1 < c.n[2] ? r2 + c.ng[2] - 1 : c.n[2];
        const unsigned m12 = s.n[1] * s.n[2], M = s.n[0] * m12, half = (M + 1) / 2;
        const double* fi = fg + (size_t)i * c.fslice;
        for (unsigned t = tid; t < half; t += nt) {
            const unsigned is[2] = {t, M - 1 - t};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned idx = is[h];
                if (h == 1 && idx == is[0]) break;  // the middle output of an odd M
                const unsigned k0 = idx / m12, q = idx - k0 * m12, k1 = q / s.n[2], k2 = q - k1 * s.n[2];
                const bool added = k0 < c.sl[0] && k1 < c.sl[1] && k2 < c.sl[2];
                V fv = E::zero();
                if (added) fv = E::ld(fi, pl.x, (size_t)k0 * c.xs[0] + (size_t)k1 * c.xs[1] + (size_t)k2 * c.xs[2]);  // in flight during the sums
                V z;
                if (GLDS) z = s3_mul_out<E>(cur, S3InLds<E>{gl, c.ng[1] * c.ng[2], c.ng[2]}, s, k0, k1, k2);
                else z = s3_mul_out<E>(cur, S3InGlobal<E>{g + o.y, pl.y, c.ys[0], c.ys[1], c.ys[2]}, s, k0, k1, k2);
                if (added) z = E::add(z, fv);
                S2L<E>::put(nxt, idx, z);
            }
        }
        lds_barrier();
        T* sw = cur;
        cur = nxt;
        nxt = sw;
        r0 = s.n[0], r1 = s.n[1], r2 = s.n[2];
    }
    __syncthreads();  // (every global load of this workgroup is done: the result may be f or g)
    const unsigned r12 = r1 * r2, total = r0 * r12;  // (r is S: series3_compose_dims walked the same steps)
    for (unsigned i = tid; i < total; i += nt) {
        const unsigned k0 = i / r12, q = i - k0 * r12, k1 = q / r2, k2 = q - k1 * r2;
        E::st(res, pl.r, o.r + (size_t)k0 * c.rs[0] + (size_t)k1 * c.rs[1] + (size_t)k2 * c.rs[2], S2L<E>::get(cur, (int)i));
    }
    s3_zero_fill<E>(res + o.r, pl.r, c);
}
template <bool GLDS>
__global__ __launch_bounds__(512) void k_series3_compose(const double* f, const double* g, double* res, Series3Compose c, SeriesBatch b) {
    extern __shared__ double s3_lds[];
    s3_compose_body<EF64, GLDS>(s3_lds, f, g, res, c, b, SeriesPlanes());
}
template <class E, bool GLDS>
__global__ __launch_bounds__(512) void k_series3i_compose(const double* f, const double* g, double* res, Series3Compose c, SeriesBatch b,
                                                          SeriesPlanes pl) {
    extern __shared__ S2Iv s3_lds_iv[];
    s3_compose_body<E, GLDS>(s3_lds_iv, f, g, res, c, b, pl);
}

// ---- div, exp, log --------------------------------------------------------------------------------------------------------------
// A is the operand resident beside the result r: div's y, exp's and log's x.  With (*) the rank-2 product of two slabs, the row sums
// of every (j1, k1 - j1) added in ascending j1 to the accumulators that already hold the earlier j0:
//   div  c = sum_{j0 = max(0,k0+1-ny0) .. k0-1} r[j0] (*) y[k0-j0];  c = -c;  c[:nx1][:nx2] += x[k0] (k0 < nx0);  r[k0] = div2(c, y[0])
//   exp  r[0] = exp2(x[0]);  c = sum_{j0 = 1 .. min(nx0,k0+1)-1} (x[j0] * j0) (*) r[k0-j0];  r[k0] = c / k0
//   log  r[0] = log2(x[0]);  c = sum_{j0 = max(1,k0+1-nx0) .. k0-1} x[k0-j0] (*) (r[j0] * j0);  c = -c;  c[:nx1][:nx2] += k0 * x[k0];
//        r[k0] = div2(c, x[0]) / k0
// div2 / exp2 / log2: the rank-2 recurrences (s2_rec_rows).  `tc`: terms per chunk; the scratch holds `selems` >= tc * n1 * n2 elements.
// `y`: div's divisor; exp / log: the seeds per item or null.  div reads its dividend slab x[k0] from global memory in the step of
// slab k0; the result is stored once at the end, so it may be x (or y) itself.
template <class E, int OP>
__device__ inline void s3_rec_body(typename S2L<E>::T* lds, const double* x, const double* y, double* res, const Series3Dims& d, unsigned tc,
                                   unsigned selems, const SeriesBatch& g, const SeriesPlanes& pl) {
    typedef typename E::V V;
    typedef typename S2L<E>::T T;  // A [a0][a1][a2] | r [n0][n1][n2] | scratch [selems]
    constexpr bool DIV = OP == SERIES_DIV, EXP = OP == SERIES_EXP;
    const unsigned* a = DIV ? d.ny : d.nx;
    const unsigned a0 = a[0], a1 = a[1], a2 = a[2], n0 = d.n[0], n1 = d.n[1], n2 = d.n[2], n12 = n1 * n2, a12 = a1 * a2;
    T* al = lds;
    T* rl = al + a0 * a12;
    T* sl = rl + n0 * n12;
    const unsigned tid = threadIdx.x, nt = blockDim.x;
    const SeriesOff o = series_offsets(g, blockIdx.x);
    if (DIV) s3_stage<E>(al, y + o.y, pl.y, d.ys, d.ny);
    else s3_stage<E>(al, x + o.x, pl.x, d.xs, d.nx);
    __syncthreads();
    // the rank-2 recurrences on a slab share the scratch (series3_plan: at least one row where a row has terms, two where the
    // dividend is in LDS)
    const unsigned terms2 = (n1 < a1 ? n1 : a1) - 1, fit = selems / n2;  // terms2: of the longest j range of a rank-2 row
    if (!DIV) {  // slab 0: the rank-2 body on slab 0 of x
        s2_rec_rows<E, OP>(al, a1, a2, rl, n1, n2, sl, terms2 < fit ? terms2 : fit, nullptr, 0, 0, 0, a1, a2, y ? y + o.s : nullptr, pl.s);
    } else if (n0 == 1) {  // one slab: the rank-2 division itself, the dividend in global memory at its two strides
        s2_rec_rows<E, OP>(al, a1, a2, rl, n1, n2, sl, terms2 < fit ? terms2 : fit, x + o.x, pl.x, d.xs[1], d.xs[2], d.nx[1], d.nx[2], nullptr, 0);
    }
    const unsigned J1 = n1 < a1 ? n1 : a1;
    for (unsigned k0 = DIV && n0 > 1 ? 0u : 1u; k0 < n0; ++k0) {
        unsigned jlo, jhi;  // the slabs j0 of the terms, ascending
        if (EXP) {
            jlo = 1;
            jhi = a0 < k0 + 1 ? a0 : k0 + 1;
        } else {
            jlo = k0 + 1 > a0 ? k0 + 1 - a0 : 0;
            if (!DIV && jlo < 1) jlo = 1;
            jhi = k0;
        }
        const unsigned T_ = jlo < jhi ? (jhi - jlo) * J1 : 0;
        T* rk = rl + k0 * n12;
        for (unsigned tb = 0; tb < T_; tb += tc) {
            const unsigned cnt = T_ - tb < tc ? T_ - tb : tc;
            // pass 1: the row sums of the chunk, one (t, k1, k2) a lane; a place of j1 that row k1 does not use stays unwritten
            for (unsigned idx = tid; idx < cnt * n12; idx += nt) {
                const unsigned tt = idx / n12, r = idx - tt * n12, k1 = r / n2, k2 = r - k1 * n2;
                const unsigned t = tb + tt, q = t / J1, j1i = t - q * J1, j0 = jlo + q;
                const unsigned cnt1 = k1 + 1 < a1 ? k1 + 1 : a1;
                if (j1i >= cnt1) continue;
                V s = E::zero();
                if (DIV) {  // mul_1d(r[j0][j1], y[k0-j0][k1-j1]): j1 from max(0, k1+1-ny1)
                    const unsigned j1 = k1 + 1 - cnt1 + j1i;
                    const T* p = rl + (j0 * n1 + j1) * n2;
                    const T* b = al + ((k0 - j0) * a1 + (k1 - j1)) * a2 + k2;
                    const unsigned lo = k2 + 1 > a2 ? k2 + 1 - a2 : 0;
#pragma unroll 4
                    for (unsigned j2 = lo; j2 <= k2; ++j2) s = E::mac(s, S2L<E>::get(p, (int)j2), S2L<E>::get(b, -(int)j2));
                } else {
                    const V fj = E::from_u32(j0);
                    const unsigned j1 = j1i, hi = k2 + 1 < a2 ? k2 + 1 : a2;
                    if (EXP) {  // mul_1d(x[j0][j1] * j0, r[k0-j0][k1-j1]): x * j0 is rounded before it meets r
                        const T* p = al + (j0 * a1 + j1) * a2;
                        const T* b = rl + ((k0 - j0) * n1 + (k1 - j1)) * n2 + k2;
#pragma unroll 4
                        for (unsigned j2 = 0; j2 < hi; ++j2) s = E::mac(s, E::mulw(S2L<E>::get(p, (int)j2), fj), S2L<E>::get(b, -(int)j2));
                    } else {  // mul_1d(x[k0-j0][j1], r[j0][k1-j1] * j0)
                        const T* p = al + ((k0 - j0) * a1 + j1) * a2;
                        const T* b = rl + (j0 * n1 + (k1 - j1)) * n2 + k2;
#pragma unroll 4
                        for (unsigned j2 = 0; j2 < hi; ++j2) s = E::mac(s, S2L<E>::get(p, (int)j2), E::mulw(S2L<E>::get(b, -(int)j2), fj));
                    }
                }
                S2L<E>::put(sl, idx, s);
            }
            lds_barrier();
            // pass 2: the ordered additions; r[k0] carries the accumulators from chunk to chunk
            for (unsigned i = tid; i < n12; i += nt) {
                const unsigned k1 = i / n2, cnt1 = k1 + 1 < a1 ? k1 + 1 : a1;
                V c = tb == 0 ? E::zero() : S2L<E>::get(rk, (int)i);
                unsigned j1i = tb % J1;
                for (unsigned tt = 0; tt < cnt; ++tt) {
                    if (j1i < cnt1) c = E::addw(c, S2L<E>::get(sl, (int)(tt * n12 + i)));
                    if (++j1i == J1) j1i = 0;
                }
                S2L<E>::put(rk, i, c);
            }
            lds_barrier();
        }
        // the slab's own step (a lane meets the coefficients it owned in pass 2)
        for (unsigned i = tid; i < n12; i += nt) {
            const unsigned k1 = i / n2, k2 = i - k1 * n2;
            V c = T_ ? S2L<E>::get(rk, (int)i) : E::zero();
            if (EXP) {
                c = E::div(c, E::from_u32(k0));
            } else {
                c = E::neg(c);
                if (k0 < d.nx[0] && k1 < d.nx[1] && k2 < d.nx[2])
                    c = E::add(c, DIV ? E::ld(x, pl.x, o.x + (size_t)k0 * d.xs[0] + (size_t)k1 * d.xs[1] + (size_t)k2 * d.xs[2])
                                      : E::mul(E::from_u32(k0), S2L<E>::get(al, (int)(k0 * a12 + k1 * a2 + k2))));
            }
            S2L<E>::put(rk, i, c);
        }
        lds_barrier();
        if (!EXP) {  // the rank-2 division of the slab, in place, by slab 0 of the resident operand
            const unsigned sr = terms2 + 1 < fit ? terms2 : (fit ? fit - 1 : 0);  // (one row of the scratch holds the accumulators)
            // (intervals: div and log share this instantiation, which the inliner then leaves a call with a scratch frame -- forced
            // at this call only, the f64 kernels compile as before)
            if constexpr (E::W == 2) [[clang::always_inline]] s2_rec_rows<E, SERIES_DIV, true>(al, a1, a2, rk, n1, n2, sl, sr, nullptr, 0, 0, 0, n1, n2, nullptr, 0);
            else s2_rec_rows<E, SERIES_DIV, true>(al, a1, a2, rk, n1, n2, sl, sr, nullptr, 0, 0, 0, n1, n2, nullptr, 0);
            if (!DIV) {
                for (unsigned i = tid; i < n12; i += nt) S2L<E>::put(rk, i, E::div(S2L<E>::get(rk, (int)i), E::from_u32(k0)));
                lds_barrier();
            }
        }
    }
    __syncthreads();  // (every global load of this workgroup is done: the result may be an operand)
    const unsigned N = n0 * n12;
    for (unsigned i = tid; i < N; i += nt) {
        const unsigned k0 = i / n12, r = i - k0 * n12, k1 = r / n2, k2 = r - k1 * n2;
        E::st(res, pl.r, o.r + (size_t)k0 * d.rs[0] + (size_t)k1 * d.rs[1] + (size_t)k2 * d.rs[2], S2L<E>::get(rl, (int)i));
    }
    s3_zero_fill<E>(res + o.r, pl.r, d);
}
template <int OP>
__global__ __launch_bounds__(256) void k_series3_rec(const double* x, const double* y, double* res, Series3Dims d, unsigned tc, unsigned selems,
                                                     SeriesBatch g) {
    extern __shared__ double s3_lds[];
    s3_rec_body<EF64, OP>(s3_lds, x, y, res, d, tc, selems, g, SeriesPlanes());
}
template <class E, int OP>
__global__ __launch_bounds__(256) void k_series3i_rec(const double* x, const double* y, double* res, Series3Dims d, unsigned tc, unsigned selems,
                                                      SeriesBatch g, SeriesPlanes pl) {
    extern __shared__ S2Iv s3_lds_iv[];
    s3_rec_body<E, OP>(s3_lds_iv, x, y, res, d, tc, selems, g, pl);
}

}  // namespace gft
