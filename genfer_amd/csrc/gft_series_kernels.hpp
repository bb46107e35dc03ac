// Device side of the batched series (gft_series.hip plans and launches these): the per-lane recurrences, form A's LDS
// staging and the kernels, as templates over the element functor (gft_elem.hpp) so that an interval twin is an instantiation.
// tests/series_isa_check.hip instantiates the form-A mul and div kernels from this file alone, tests/series_compose_isa_check.hip
// the two compose kernels, tests/series_corr_isa_check.hip the transposed products (corr forms A and B, compose_adj).
#pragma once
#include <hip/hip_runtime.h>

#include "gft_elem.hpp"
#include "gft_series.hpp"

namespace gft {

template <class E>
struct RowLds {  // lane's row in a wave's LDS array: [plane][64 * pitch]
    double* p;
    size_t plane;
    __device__ typename E::V ld(unsigned i) const { return E::ld(p, plane, i); }
    __device__ void st(unsigned i, typename E::V v) const { E::st(p, plane, i, v); }
};
template <class E>
struct ColWs {  // item's column of a transposed workspace: [plane][n][items]
    double* p;
    size_t plane, items;
    __device__ typename E::V ld(unsigned i) const { return E::ld(p, plane, (size_t)i * items); }
    __device__ void st(unsigned i, typename E::V v) const { E::st(p, plane, (size_t)i * items, v); }
};

// The reference's product does not store the sums of mul_1d: mul_rec adds them onto the zeroed result, z[k] = z[k] + out[k] with
// z[k] == 0 (mt:984-1012).  Where zero is neutral (F64: a sum formed from +0 is never -0; Interval<F64>: [0,0] + b returns b) that
// addition returns its operand and the kernels never performed it.  BigFloat's {0, 0} + s rescales s by powi(2, s.exponent), which
// changes s at exponent -1023 and drops it below: there the addition is performed (EBig::add0).  The sums of div, exp and log are
// stored as they are formed (mt:1162-1192, 1271-1283, 1319-1333): no such addition there.
template <class E>
__device__ inline typename E::V onto_zero(typename E::V sum) {
    if constexpr (E::ZERO_NEUTRAL) return sum;
    else return E::add0(sum);
}

// ---- the recurrences, one series per lane (the loops of k_exp_1d / k_log_1d / k_div_1d_serial / k_conv_* reference order) ----
// z[k] = 0 + sum_{j = lo .. hi-1} x[j] * y[k-j], ascending j (mul_1d, mt:972-982).  k runs downwards and z[k] overwrites y[k]:
// the outputs still to come read y[0 .. k-1] only.
template <class E, class AX, class AY>
__device__ inline void rec_mul(const AX x, const AY y, unsigned nx, unsigned ny, unsigned n) {
    typedef typename E::V V;
    for (unsigned k = n; k-- > 0;) {
        const unsigned lo = k + 1 > ny ? k + 1 - ny : 0, hi = k + 1 < nx ? k + 1 : nx;
        V sum = E::zero();
#pragma unroll 4
        for (unsigned j = lo; j < hi; ++j) sum = E::add(sum, E::mul(x.ld(j), y.ld(k - j)));
        y.st(k, onto_zero<E>(sum));
    }
}
// One Horner step of compose in place: r <- r * g truncated at L <= lr + ng - 1, r holding lr coefficients on entry (the same sums as
// rec_mul with x = r; here z[k] overwrites x[k], which the outputs still to come, reading r[0 .. k-1], do not need).
template <class E, class AR, class AG>
__device__ inline void rec_horner_step(const AR r, const AG g, unsigned lr, unsigned ng, unsigned L) {
    typedef typename E::V V;
    for (unsigned k = L; k-- > 0;) {
        const unsigned lo = k + 1 > ng ? k + 1 - ng : 0, hi = k + 1 < lr ? k + 1 : lr;
        V sum = E::zero();
#pragma unroll 4
        for (unsigned j = lo; j < hi; ++j) sum = E::add(sum, E::mul(r.ld(j), g.ld(k - j)));
        r.st(k, onto_zero<E>(sum));
    }
}
// The transposed product, c[i] = 0 + sum_k g[k] * y[k-i] with k DESCENDING from min(ng-1, i+ny-1) to i: the sums of mul_1d on the
// flipped row, z = flip(g) * y at index ng-1-i in ascending j = ng-1-k, so <mul(x, y), g> = <x, corr(g, y)> term for term.  i runs
// upwards and c[i] overwrites g[i]: the outputs still to come read g[i+1 ..] only.
template <class E, class AG, class AY>
__device__ inline void rec_corr(const AG g, const AY y, unsigned ng, unsigned ny, unsigned m) {
    typedef typename E::V V;
    for (unsigned i = 0; i < m; ++i) {
        const unsigned top = ng - i < ny ? ng - i : ny;  // terms of this output
        V sum = E::zero();
#pragma unroll 4
        for (unsigned d = top; d-- > 0;) sum = E::add(sum, E::mul(g.ld(i + d), y.ld(d)));
        g.st(i, sum);
    }
}
// r[k] = (-(0 + sum_{j = lo .. k-1} r[j] * y[k-j]) + x[k]) / y[0] (div, mt:1162-1192 at one axis); r holds x on entry.
template <class E, class AY, class AR>
__device__ inline void rec_div(const AY y, const AR r, unsigned nx, unsigned ny, unsigned n) {
    typedef typename E::V V;
    const V y0 = y.ld(0);
    for (unsigned k = 0; k < n; ++k) {
        const unsigned lo = k + 1 > ny ? k + 1 - ny : 0;
        V sum = E::zero();
#pragma unroll 4
        for (unsigned j = lo; j < k; ++j) sum = E::add(sum, E::mul(r.ld(j), y.ld(k - j)));
        V c = E::neg(sum);
        if (k < nx) c = E::add(c, r.ld(k));
        r.st(k, E::div(c, y0));
    }
}
// exp_1d, mt:1271-1283
template <class E, class AX, class AR>
__device__ inline void rec_exp(const AX x, const AR r, unsigned nx, unsigned n, typename E::V seed) {
    typedef typename E::V V;
    r.st(0, seed);
    for (unsigned k = 1; k < n; ++k) {
        const unsigned hi = nx < k + 1 ? nx : k + 1;
        V sum = E::zero();
#pragma unroll 4
        for (unsigned j = 1; j < hi; ++j) sum = E::add(sum, E::mul(E::mul(x.ld(j), E::from_u32(j)), r.ld(k - j)));
        r.st(k, E::div(sum, E::from_u32(k)));
    }
}
// log_1d, mt:1319-1333.  A one-coefficient operand has no higher orders: they are written as +0 (the reference stores none).
template <class E, class AX, class AR>
__device__ inline void rec_log(const AX x, const AR r, unsigned nx, unsigned n, typename E::V seed) {
    typedef typename E::V V;
    const V x0 = x.ld(0);
    r.st(0, seed);
    for (unsigned k = 1; k < n; ++k) {
        if (nx == 1) {
            r.st(k, E::zero());
            continue;
        }
        unsigned lo = k + 1 > nx ? k + 1 - nx : 0;
        if (lo < 1) lo = 1;
        V sum = E::zero();
#pragma unroll 4
        for (unsigned j = lo; j < k; ++j) sum = E::add(sum, E::mul(E::mul(x.ld(k - j), r.ld(j)), E::from_u32(j)));
        const V xk = k < nx ? x.ld(k) : E::zero();
        const V num = E::sub(E::mul(xk, E::from_u32(k)), sum);
        r.st(k, E::div(E::div(num, x0), E::from_u32(k)));
    }
}

// ---- form A staging ---------------------------------------------------------------------------------------------------------
// The wave's 64 rows of `len` elements between global memory (row l at base + off_l, planes gp apart) and LDS (row l at
// l * pitch, planes lp apart).  A group of 2^lg lanes walks one row, 64 >> lg rows per pass; every lane runs the same number
// of passes (the row offset of pass t comes from its owner lane by a shuffle, which all lanes execute).
template <class E, bool IN>
__device__ inline void stage_rows(double* lds, size_t lp, unsigned pitch, double* gptr, size_t gp, size_t my_off, unsigned len,
                                  unsigned lg, unsigned item0, unsigned items, unsigned lane) {
    const unsigned G = 1u << lg, per = 64u >> lg, sub = lane >> lg, i0 = lane & (G - 1);
    for (unsigned t = 0; t < G; ++t) {
        const unsigned l = t * per + sub;
        const size_t off = (size_t)__shfl((unsigned long long)my_off, (int)l, 64);
        if (item0 + l >= items) continue;
        for (unsigned i = i0; i < len; i += G) {
#pragma unroll
            for (int w = 0; w < E::W; ++w) {
                if (IN) lds[w * lp + l * pitch + i] = gptr[w * gp + off + i];
                else gptr[w * gp + off + i] = lds[w * lp + l * pitch + i];
            }
        }
    }
}

struct FormA {  // what every form-A kernel derives from its thread index
    unsigned lane, item0, it;
    size_t lp;       // LDS plane stride: 64 * pitch
    double *a0, *a1;  // the wave's first two arrays (compose has a third behind them)
};
template <class E>
__device__ inline FormA form_a(double* lds, unsigned pitch, unsigned items, unsigned arrays = 2) {
    FormA f;
    const unsigned wave = threadIdx.x >> 6;
    f.lane = threadIdx.x & 63;
    f.lp = (size_t)64 * pitch;
    f.a0 = lds + (size_t)wave * arrays * E::W * f.lp;
    f.a1 = f.a0 + E::W * f.lp;
    f.item0 = (blockIdx.x * (blockDim.x >> 6) + wave) * 64;
    f.it = f.item0 + f.lane < items ? f.item0 + f.lane : items - 1;  // a lane past the batch: valid addresses, an unstaged row, nothing stored
    return f;
}

template <class E>
__global__ __launch_bounds__(256) void k_series_mul_a(const double* x, size_t xp, unsigned nx, const double* y, size_t yp, unsigned ny,
                                                      double* res, size_t rp, unsigned n, unsigned pitch, unsigned lg, SeriesBatch g) {
    extern __shared__ double sa_lds[];
    const FormA f = form_a<E>(sa_lds, pitch, g.items);
    const SeriesOff o = series_offsets(g, f.it);
    stage_rows<E, true>(f.a0, f.lp, pitch, const_cast<double*>(x), xp, o.x, nx, lg, f.item0, g.items, f.lane);
    stage_rows<E, true>(f.a1, f.lp, pitch, const_cast<double*>(y), yp, o.y, ny, lg, f.item0, g.items, f.lane);
    __syncthreads();
    rec_mul<E>(RowLds<E>{f.a0 + f.lane * pitch, f.lp}, RowLds<E>{f.a1 + f.lane * pitch, f.lp}, nx, ny, n);
    __syncthreads();
    stage_rows<E, false>(f.a1, f.lp, pitch, res, rp, o.r, n, lg, f.item0, g.items, f.lane);
}

template <class E>
__global__ __launch_bounds__(256) void k_series_div_a(const double* x, size_t xp, unsigned nx, const double* y, size_t yp, unsigned ny,
                                                      double* res, size_t rp, unsigned n, unsigned pitch, unsigned lg, SeriesBatch g) {
    extern __shared__ double sa_lds[];
    const FormA f = form_a<E>(sa_lds, pitch, g.items);
    const SeriesOff o = series_offsets(g, f.it);
    stage_rows<E, true>(f.a0, f.lp, pitch, const_cast<double*>(y), yp, o.y, ny, lg, f.item0, g.items, f.lane);
    stage_rows<E, true>(f.a1, f.lp, pitch, const_cast<double*>(x), xp, o.x, nx, lg, f.item0, g.items, f.lane);
    __syncthreads();
    rec_div<E>(RowLds<E>{f.a0 + f.lane * pitch, f.lp}, RowLds<E>{f.a1 + f.lane * pitch, f.lp}, nx, ny, n);
    __syncthreads();
    stage_rows<E, false>(f.a1, f.lp, pitch, res, rp, o.r, n, lg, f.item0, g.items, f.lane);
}

// corr, c = the transposed product of g (ng coefficients) and y (ny <= ng), m <= ng outputs: c overwrites g's row from the bottom up
template <class E>
__global__ __launch_bounds__(256) void k_series_corr_a(const double* g, size_t gp, unsigned ng, const double* y, size_t yp, unsigned ny,
                                                       double* res, size_t rp, unsigned m, unsigned pitch, unsigned lg, SeriesBatch b) {
    extern __shared__ double sa_lds[];
    const FormA f = form_a<E>(sa_lds, pitch, b.items);
    const SeriesOff o = series_offsets(b, f.it);
    stage_rows<E, true>(f.a0, f.lp, pitch, const_cast<double*>(g), gp, o.x, ng, lg, f.item0, b.items, f.lane);
    stage_rows<E, true>(f.a1, f.lp, pitch, const_cast<double*>(y), yp, o.y, ny, lg, f.item0, b.items, f.lane);
    __syncthreads();
    rec_corr<E>(RowLds<E>{f.a0 + f.lane * pitch, f.lp}, RowLds<E>{f.a1 + f.lane * pitch, f.lp}, ng, ny, m);
    __syncthreads();
    stage_rows<E, false>(f.a0, f.lp, pitch, res, rp, o.r, m, lg, f.item0, b.items, f.lane);
}

// exp (LOG == false) / log: `seed` holds exp(x[0]) / ln(x[0]) per item, or is null: formed here by the device library
template <class E, bool LOG>
__global__ __launch_bounds__(256) void k_series_explog_a(const double* x, size_t xp, unsigned nx, const double* seed, size_t sp,
                                                         double* res, size_t rp, unsigned n, unsigned pitch, unsigned lg, SeriesBatch g) {
    extern __shared__ double sa_lds[];
    const FormA f = form_a<E>(sa_lds, pitch, g.items);
    const SeriesOff o = series_offsets(g, f.it);
    stage_rows<E, true>(f.a0, f.lp, pitch, const_cast<double*>(x), xp, o.x, nx, lg, f.item0, g.items, f.lane);
    __syncthreads();
    const RowLds<E> xr{f.a0 + f.lane * pitch, f.lp}, rr{f.a1 + f.lane * pitch, f.lp};
    const typename E::V sd = seed ? E::ld(seed, sp, o.s) : (LOG ? E::log(xr.ld(0)) : E::exp(xr.ld(0)));
    if (LOG) rec_log<E>(xr, rr, nx, n, sd);
    else rec_exp<E>(xr, rr, nx, n, sd);
    __syncthreads();
    stage_rows<E, false>(f.a1, f.lp, pitch, res, rp, o.r, n, lg, f.item0, g.items, f.lane);
}

// compose, res = f(g) by Horner (subst_var's general path, mt:574-578, with mul_1d at every step): three arrays per wave, f, g and
// the result row, whose compact length lr grows by ng - 1 a step up to n (sum_shape, mt:150-170) -- the same in every lane.
template <class E>
__global__ __launch_bounds__(256) void k_series_compose_a(const double* f, size_t fp, unsigned nf, const double* g, size_t gp, unsigned ng,
                                                          double* res, size_t rp, unsigned n, unsigned pitch, unsigned lg, SeriesBatch b) {
    extern __shared__ double sa_lds[];
    const FormA a = form_a<E>(sa_lds, pitch, b.items, 3);
    double* a2 = a.a1 + E::W * a.lp;
    const SeriesOff o = series_offsets(b, a.it);
    stage_rows<E, true>(a.a0, a.lp, pitch, const_cast<double*>(f), fp, o.x, nf, lg, a.item0, b.items, a.lane);
    stage_rows<E, true>(a.a1, a.lp, pitch, const_cast<double*>(g), gp, o.y, ng, lg, a.item0, b.items, a.lane);
    __syncthreads();
    const RowLds<E> fr{a.a0 + a.lane * pitch, a.lp}, gr{a.a1 + a.lane * pitch, a.lp}, rr{a2 + a.lane * pitch, a.lp};
    unsigned lr = 1;
    rr.st(0, E::add(E::zero(), fr.ld(nf - 1)));
    for (unsigned i = nf - 1; i-- > 0;) {
        const unsigned L = lr + ng - 1 < n ? lr + ng - 1 : n;
        rec_horner_step<E>(rr, gr, lr, ng, L);
        rr.st(0, E::add(rr.ld(0), fr.ld(i)));
        lr = L;
    }
    for (unsigned k = lr; k < n; ++k) rr.st(k, E::zero());
    __syncthreads();
    stage_rows<E, false>(a2, a.lp, pitch, res, rp, o.r, n, lg, a.item0, b.items, a.lane);
}

// ---- form B ---------------------------------------------------------------------------------------------------------------
// mul: blockIdx.x is the item, blockIdx.y a share of its outputs.  A thread owns the outputs k1 = t and k2 = n - 1 - t, together
// n + 1 terms whatever t, each sum formed from +0 in ascending j over the stored operands only (the bounds of mul_1d).  Within a
// wave j runs in step, so x[j] is one LDS address for the wave and y[k - j] consecutive across lanes.  A series may be shared
// by several workgroups only when `res` is neither x nor y (g.inplace == 0): each stages the whole row pair before it stores.
template <class E>
__global__ __launch_bounds__(256) void k_series_mul_b(const double* x, size_t xp, unsigned nx, const double* y, size_t yp, unsigned ny,
                                                      double* res, size_t rp, unsigned n, SeriesBatch g) {
    typedef typename E::V V;
    extern __shared__ double sb_lds[];  // [plane][nx] | [plane][ny]
    double* xl = sb_lds;
    double* yl = sb_lds + (size_t)E::W * nx;
    const SeriesOff o = series_offsets(g, blockIdx.x);
    for (unsigned i = threadIdx.x; i < nx; i += blockDim.x) E::st(xl, nx, i, E::ld(x + o.x, xp, i));
    for (unsigned i = threadIdx.x; i < ny; i += blockDim.x) E::st(yl, ny, i, E::ld(y + o.y, yp, i));
    __syncthreads();  // (every global load of this workgroup is done)
    const unsigned half = (n + 1) / 2;
    for (unsigned t = blockIdx.y * blockDim.x + threadIdx.x; t < half; t += gridDim.y * blockDim.x) {
        const unsigned ks[2] = {t, n - 1 - t};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned k = ks[h];
            if (h == 1 && k == ks[0]) break;  // the middle output of an odd n
            const unsigned lo = k + 1 > ny ? k + 1 - ny : 0, hi = k + 1 < nx ? k + 1 : nx;
            V sum = E::zero();
#pragma unroll 4
            for (unsigned j = lo; j < hi; ++j) sum = E::add(sum, E::mul(E::ld(xl, nx, j), E::ld(yl, ny, k - j)));
            E::st(res + o.r, rp, k, onto_zero<E>(sum));
        }
    }
}

// compose: blockIdx.x is the item, and the whole Horner loop runs in this one workgroup (the steps are a dependency chain).  Two
// result rows in LDS take turns (a step reads one and writes the other) and g sits behind them (GLDS) or stays in global memory
// (the 64 KB fallback for long rows).  Every step is mul form B's truncated product at the compact length L: a thread owns the
// outputs t and L - 1 - t, and the owner of output 0 adds f[i], its only global load of the step.  Between steps the threads meet
// through LDS alone.  A result in place is safe: this workgroup has read all of f and g before its first store.
template <class E, bool GLDS>
__global__ __launch_bounds__(256) void k_series_compose_b(const double* f, size_t fp, unsigned nf, const double* g, size_t gp, unsigned ng,
                                                          double* res, size_t rp, unsigned n, SeriesBatch b) {
    typedef typename E::V V;
    extern __shared__ double sb_lds[];  // [plane][n] | [plane][n] | [plane][ng]
    double* r0 = sb_lds;
    double* r1 = sb_lds + (size_t)E::W * n;
    const SeriesOff o = series_offsets(b, blockIdx.x);
    const double* fg = f + o.x;
    const double* gsrc = g + o.y;
    size_t gplane = gp;
    if (GLDS) {
        double* gl = sb_lds + (size_t)2 * E::W * n;
        for (unsigned i = threadIdx.x; i < ng; i += blockDim.x) E::st(gl, ng, i, E::ld(g + o.y, gp, i));
        gsrc = gl;
        gplane = ng;
    }
    if (threadIdx.x == 0) E::st(r0, n, 0, E::add(E::zero(), E::ld(fg, fp, nf - 1)));
    __syncthreads();
    unsigned lr = 1;
    for (unsigned i = nf - 1; i-- > 0;) {
        const unsigned L = lr + ng - 1 < n ? lr + ng - 1 : n, half = (L + 1) / 2;
        for (unsigned t = threadIdx.x; t < half; t += blockDim.x) {
            V fi = E::zero();
            if (t == 0) fi = E::ld(fg, fp, i);  // in flight during the sums below
            const unsigned ks[2] = {t, L - 1 - t};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned k = ks[h];
                if (h == 1 && k == ks[0]) break;  // the middle output of an odd L
                const unsigned lo = k + 1 > ng ? k + 1 - ng : 0, hi = k + 1 < lr ? k + 1 : lr;
                V sum = E::zero();
#pragma unroll 4
                for (unsigned j = lo; j < hi; ++j) sum = E::add(sum, E::mul(E::ld(r0, n, j), E::ld(gsrc, gplane, k - j)));
                sum = onto_zero<E>(sum);
                if (k == 0) sum = E::add(sum, fi);
                E::st(r1, n, k, sum);
            }
        }
        lds_barrier();
        double* sw = r0;
        r0 = r1;
        r1 = sw;
        lr = L;
    }
    __syncthreads();  // (every global load of this workgroup is done: the result may be f or g)
    for (unsigned k = threadIdx.x; k < n; k += blockDim.x) E::st(res + o.r, rp, k, k < lr ? E::ld(r0, n, k) : E::zero());
}

// ---- the transposed product in form B -------------------------------------------------------------------------------------------
// One output of corr over a staged row pair: c[i] = 0 + sum_d g[i+d] * y[d], d = k - i descending.  The wave walks d in lock step
// from the highest offset any of its outputs [i_lo, i_hi] has, so y[d] is one address for the wave and g[i+d] consecutive across
// lanes; a lane whose row ends below i + d forms no term and performs no addition (down to d_all every lane has one: no guard).
// i_lo, i_hi are the same in every lane of the wave.
template <class E>
__device__ inline typename E::V corr_sum(const double* gl, size_t gplane, unsigned ng, const double* yl, size_t yplane, unsigned ny,
                                         unsigned i, unsigned i_lo, unsigned i_hi) {
    typedef typename E::V V;
    const unsigned top = ng - i_lo < ny ? ng - i_lo : ny, all = ng - i_hi < ny ? ng - i_hi : ny;  // offsets below: some lane's, every lane's
    const unsigned d_top = __builtin_amdgcn_readfirstlane(top), d_all = __builtin_amdgcn_readfirstlane(all);
    V sum = E::zero();
    unsigned d = d_top;
    for (; d > d_all; --d)
        if (i + d - 1 < ng) sum = E::add(sum, E::mul(E::ld(gl, gplane, i + d - 1), E::ld(yl, yplane, d - 1)));
#pragma unroll 4
    for (; d > 0; --d) sum = E::add(sum, E::mul(E::ld(gl, gplane, i + d - 1), E::ld(yl, yplane, d - 1)));
    return sum;
}
// The outputs of one wave's turn: thread t owns i = t and i = m - 1 - t (together about the same number of terms whatever t), t
// counted from the wave's t0 and below `half` = (m + 1) / 2.  fn(i, sum) stores.
template <class E, class F>
__device__ inline void corr_pairs(const double* gl, size_t gplane, unsigned ng, const double* yl, size_t yplane, unsigned ny, unsigned m,
                                  unsigned half, unsigned t0, unsigned lane, F fn) {
    const unsigned t = t0 + lane, last = t0 + 63 < half ? t0 + 63 : half - 1;
    if (t >= half) return;
    fn(t, corr_sum<E>(gl, gplane, ng, yl, yplane, ny, t, t0, last));
    const unsigned i = m - 1 - t;
    if (i != t) fn(i, corr_sum<E>(gl, gplane, ng, yl, yplane, ny, i, m - 1 - last, m - 1 - t0));  // (not the middle output of an odd m again)
}

// corr: blockIdx.x is the item, blockIdx.y a share of its outputs, as in k_series_mul_b.  A series may be shared by several
// workgroups only when `res` is not g (b.inplace == 0): each stages the whole row pair before it stores.
template <class E>
__global__ __launch_bounds__(256) void k_series_corr_b(const double* g, size_t gp, unsigned ng, const double* y, size_t yp, unsigned ny,
                                                       double* res, size_t rp, unsigned m, SeriesBatch b) {
    extern __shared__ double sb_lds[];  // [plane][ng] | [plane][ny]
    double* gl = sb_lds;
    double* yl = sb_lds + (size_t)E::W * ng;
    const SeriesOff o = series_offsets(b, blockIdx.x);
    for (unsigned i = threadIdx.x; i < ng; i += blockDim.x) E::st(gl, ng, i, E::ld(g + o.x, gp, i));
    for (unsigned i = threadIdx.x; i < ny; i += blockDim.x) E::st(yl, ny, i, E::ld(y + o.y, yp, i));
    __syncthreads();  // (every global load of this workgroup is done)
    const unsigned half = (m + 1) / 2, lane = threadIdx.x & 63;
    for (unsigned t0 = blockIdx.y * blockDim.x + (threadIdx.x - lane); t0 < half; t0 += gridDim.y * blockDim.x)
        corr_pairs<E>(gl, ng, ng, yl, ny, ny, m, half, t0, lane, [&](unsigned i, typename E::V sum) { E::st(res + o.r, rp, i, sum); });
}

// compose_adj, the transposed Horner loop (the gradient of compose with respect to f): a_0 = gh[0 .. l_0), out[i] = a_i[0],
// a_{i+1} = corr(a_i, g) at the compact lengths l_i = min(1 + (nf-1-i)(ng-1), n) of the forward loop run backwards.  The mirror of
// k_series_compose_b: one workgroup per series for the whole loop, two rows in LDS taking turns, g behind them (GLDS) or in global
// memory (the 64 KB fallback), steps separated by an LDS-only barrier; the owner of output 0 stores out[i+1].  gh and (GLDS) g are
// read completely before the first store, so the result may be gh itself; it is never g (the host refuses that).
template <class E, bool GLDS>
__global__ __launch_bounds__(256) void k_series_compose_adj_b(const double* gh, size_t hp, unsigned n, const double* g, size_t gp, unsigned ng,
                                                              double* res, size_t rp, unsigned nf, SeriesBatch b) {
    extern __shared__ double sb_lds[];  // [plane][l0] | [plane][l0] | [plane][ng]
    const unsigned full = (nf - 1) * (ng - 1) + 1, l0 = full < n ? full : n;
    double* r0 = sb_lds;
    double* r1 = sb_lds + (size_t)E::W * l0;
    const SeriesOff o = series_offsets(b, blockIdx.x);
    const double* gsrc = g + o.y;
    size_t gplane = gp;
    if (GLDS) {
        double* gl = sb_lds + (size_t)2 * E::W * l0;
        for (unsigned i = threadIdx.x; i < ng; i += blockDim.x) E::st(gl, ng, i, E::ld(g + o.y, gp, i));
        gsrc = gl;
        gplane = ng;
    }
    for (unsigned i = threadIdx.x; i < l0; i += blockDim.x) E::st(r0, l0, i, E::ld(gh + o.x, hp, i));
    __syncthreads();  // (every global load of gh is done)
    if (threadIdx.x == 0) E::st(res + o.r, rp, 0, E::ld(r0, l0, 0));
    const unsigned lane = threadIdx.x & 63, w0 = threadIdx.x - lane;
    unsigned li = l0;
    for (unsigned i = 0; i + 1 < nf; ++i) {
        const unsigned rest = (nf - 2 - i) * (ng - 1) + 1, ln = rest < n ? rest : n, half = (ln + 1) / 2;  // l_{i+1}
        for (unsigned t0 = w0; t0 < half; t0 += blockDim.x)
            corr_pairs<E>(r0, l0, li, gsrc, gplane, ng, ln, half, t0, lane, [&](unsigned p, typename E::V sum) {
                E::st(r1, l0, p, sum);
                if (p == 0) E::st(res + o.r, rp, i + 1, sum);
            });
        lds_barrier();
        double* sw = r0;
        r0 = r1;
        r1 = sw;
        li = ln;
    }
}

// exp / log over the transposed workspace: xT [nx][items], rT [n][items], one lane per item
template <class E, bool LOG>
__global__ __launch_bounds__(64) void k_series_explog_ws(double* xT, unsigned nx, const double* seed, size_t sp, double* rT, unsigned n,
                                                         SeriesBatch g) {
    const unsigned it = blockIdx.x * 64 + threadIdx.x;
    if (it >= g.items) return;
    const size_t items = g.items;
    const ColWs<E> xc{xT + it, (size_t)nx * items, items}, rc{rT + it, (size_t)n * items, items};
    const typename E::V sd = seed ? E::ld(seed, sp, series_offsets(g, it).s) : (LOG ? E::log(xc.ld(0)) : E::exp(xc.ld(0)));
    if (LOG) rec_log<E>(xc, rc, nx, n, sd);
    else rec_exp<E>(xc, rc, nx, n, sd);
}

}  // namespace gft
