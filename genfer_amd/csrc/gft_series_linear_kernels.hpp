// The kernels of the batched affine substitutions mul_linear and compose_linear (gft_series_linear.hip states the layout and the two
// forms; tests/series_linear_isa_check.hip instantiates them from this file alone).  Templates over the element functor: EF64, EIv,
// with the literal E::mul / E::add: a multiply and an add are rounded separately, an absent term is absent.
#pragma once
#include <hip/hip_runtime.h>

#include "gft_elem.hpp"
#include "gft_series.hpp"
#include "gft_series_observe_kernels.hpp"  // obs_shfl, obs_split

namespace gft {

constexpr unsigned LIN_THREADS_A = 256;  // form A and the streaming kernel: four waves
constexpr unsigned LIN_THREADS_B = 512;  // form B: the most lanes of a workgroup

// The lines of a call, along the axis w of the affine series.  The result of an item has `lines` of them (its length on the other
// axis; rank 1: one) of `n` coefficients; the first `live` hold coefficients, the others are +0.0.  Line j of the operand starts
// j * xline elements into the item, its coefficients are xel elements apart and slice i of it (compose_linear: index i along var)
// starts i * xslice further on; the result: rline, rel.
//   compose_linear, wvar == var: a slice of a line is ONE coefficient (slen = 1, xslice = xel), live = the operand's other length
//   compose_linear, wvar != var: one live line, a slice is a row or column of f (slen = its length on wvar)
//   mul_linear:                  slices = 1, slen = the operand's length on the axis, live = its other length
struct LinCall {
    unsigned lines, live, n, slen, slices;
    int power;  // wvar == var: an item with c == 0 takes the power table (mt:557-565)
    size_t xline, xel, xslice, rline, rel;
};

// one coefficient of mul_linear (mt:611-623) at position j of a line of stored length len, for j < min(n, len + 1): lo = a[j - 1]
// (read where j >= 1), cur = a[j] (read where j < len)
template <class E>
__device__ __forceinline__ typename E::V lin_step(typename E::V lo, typename E::V cur, unsigned j, unsigned len, typename E::V c, typename E::V m,
                                                  bool c0) {
    typedef typename E::V V;
    const V t = j == 0 ? E::zero() : E::mul(lo, m);
    if (c0 || j >= len) return t;
    return E::add(t, E::mul(c, cur));
}

// what a line needs of its item
template <class E>
struct LinLine {
    typename E::V c, m;
    bool c0, live;
    const double* src;
    double* dst;
};
template <class E>
__device__ __forceinline__ LinLine<E> lin_line(size_t line, const LinCall& q, const SeriesBatch& g, const double* a, const double* cs, size_t cp,
                                               const double* ms, size_t mp, double* res) {
    const size_t qi = line / q.lines;
    const unsigned j = (unsigned)(line - qi * q.lines);
    const SeriesOff o = series_offsets(g, (unsigned)qi);
    LinLine<E> l;
    l.live = j < q.live;
    l.src = a + o.x + (l.live ? (size_t)j * q.xline : 0);
    l.dst = res + o.r + (size_t)j * q.rline;
    l.c = E::ld(cs, cp, o.y);
    l.m = E::ld(ms, mp, o.s);
    l.c0 = E::is_zero(l.c);
    return l;
}

// mul_linear: one thread per coefficient of the result, grid-stride (k_obs_scale's shape)
template <class E>
__global__ void __launch_bounds__(LIN_THREADS_A) k_lin_mul(const double* __restrict__ a, size_t ap, const double* __restrict__ cs, size_t cp,
                                                          const double* __restrict__ ms, size_t mp, double* __restrict__ res, size_t rp, LinCall q,
                                                          SeriesBatch g) {
    typedef typename E::V V;
    const unsigned per = q.lines * q.n;
    const size_t total = (size_t)g.items * per;
    const bool narrow = total <= 0xffffffffull;
    const unsigned keep = q.n < q.slen + 1 ? q.n : q.slen + 1;  // L'
    for (size_t lin = blockIdx.x * (size_t)blockDim.x + threadIdx.x; lin < total; lin += (size_t)gridDim.x * blockDim.x) {
        unsigned it, rem;
        obs_split(lin, per, narrow, it, rem);
        const unsigned r = rem / q.n, j = rem - r * q.n;
        const SeriesOff o = series_offsets(g, it);
        V out = E::zero();
        if (r < q.live && j < keep) {
            const double* src = a + o.x + (size_t)r * q.xline;
            const V c = E::ld(cs, cp, o.y), m = E::ld(ms, mp, o.s);
            const V lo = j >= 1 ? E::ld(src, ap, (size_t)(j - 1) * q.xel) : E::zero();
            const V cur = j < q.slen ? E::ld(src, ap, (size_t)j * q.xel) : E::zero();
            out = lin_step<E>(lo, cur, j, q.slen, c, m, E::is_zero(c));
        }
        E::st(res, rp, o.r + (size_t)r * q.rline + (size_t)j * q.rel, out);
    }
}

// compose_linear, form A: one wave per line of at most 64 coefficients, lane j owns position j for the whole loop.  res[j - 1] comes
// from the previous lane; no LDS, no barrier.  The slice a step adds is loaded one step ahead.  The lanes at and above the stored
// length carry values nobody reads.
template <class E>
__global__ void __launch_bounds__(LIN_THREADS_A) k_lin_compose_wave(const double* __restrict__ f, size_t fp, const double* __restrict__ cs, size_t cp,
                                                                   const double* __restrict__ ms, size_t mp, double* __restrict__ res, size_t rp,
                                                                   LinCall q, SeriesBatch g) {
    typedef typename E::V V;
    const unsigned j = threadIdx.x & 63;
    const size_t total = (size_t)g.items * q.lines, waves = (size_t)gridDim.x * (LIN_THREADS_A / 64);
    // (a wave is one line: its trip counts, c and m are uniform, so the cross-lane reads are never divergent)
    for (size_t line = (size_t)blockIdx.x * (LIN_THREADS_A / 64) + (threadIdx.x >> 6); line < total; line += waves) {
        const LinLine<E> l = lin_line<E>(line, q, g, f, cs, cp, ms, mp, res);
        V cur = E::zero();
        unsigned len = 0;
        if (l.live) {
            const bool has = j < q.slen;
            const double* sl = l.src + (size_t)j * q.xel;  // this lane's coefficient of a slice (read where `has`)
            if (q.power && l.c0) {  // slice i times p_i, p_0 = 1, p_{i+1} = p_i * m: lane i takes i steps of the table
                len = q.slices;
                V p = E::one();
                for (unsigned i = 0; i + 1 < q.slices; ++i)
                    if (i < j) p = E::mul(p, l.m);
                if (j < len) cur = E::mul(E::ld(l.src, fp, (size_t)j * q.xslice), p);
            } else {
                len = q.slen;
                V nxt = E::zero();
                if (has) cur = E::add(E::zero(), E::ld(sl, fp, (size_t)(q.slices - 1) * q.xslice));
                if (has && q.slices >= 2) nxt = E::ld(sl, fp, (size_t)(q.slices - 2) * q.xslice);
                for (unsigned i = q.slices - 1; i-- > 0;) {
                    const V s = nxt;
                    if (has && i >= 1) nxt = E::ld(sl, fp, (size_t)(i - 1) * q.xslice);  // the next step's slice: its latency runs beside this step
                    const V lo = obs_shfl<V>(cur, (int)((j + 63) & 63));
                    V r = lin_step<E>(lo, cur, j, len, l.c, l.m, l.c0);
                    len = len + 1 < q.n ? len + 1 : q.n;
                    if (has) r = E::add(r, s);
                    cur = r;
                }
            }
        }
        if (j < q.n) E::st(l.dst, rp, (size_t)j * q.rel, j < len ? cur : E::zero());
    }
}

// compose_linear, form B: one workgroup per line, two line buffers of `pad` elements in LDS taking turns (a step reads what the one
// before wrote and the last one writes the result), an LDS-only barrier between the steps.  Where a slice is one coefficient, only
// position 0 takes it: the first wave holds the next 64 of them in registers, a lane each, loaded 64 steps ahead, and a step reads
// its own across the lanes -- no step waits for global memory.  A longer slice is loaded by the threads that add it, at the head of
// the step.
template <class E>
__global__ void __launch_bounds__(LIN_THREADS_B) k_lin_compose_lds(const double* __restrict__ f, size_t fp, const double* __restrict__ cs, size_t cp,
                                                                  const double* __restrict__ ms, size_t mp, double* __restrict__ res, size_t rp,
                                                                  LinCall q, SeriesBatch g, unsigned pad) {
    typedef typename E::V V;
    extern __shared__ double lin_lds[];
    const size_t total = (size_t)g.items * q.lines;
    const unsigned k0 = threadIdx.x, nt = blockDim.x;
    const bool wave0 = k0 < 64;  // (uniform over a wave)
    for (size_t line = blockIdx.x; line < total; line += gridDim.x) {
        const LinLine<E> l = lin_line<E>(line, q, g, f, cs, cp, ms, mp, res);
        double* buf0 = lin_lds;
        double* buf1 = lin_lds + (size_t)E::W * pad;
        if (!l.live) {
            for (unsigned k = k0; k < q.n; k += nt) E::st(l.dst, rp, (size_t)k * q.rel, E::zero());
            continue;
        }
        if (q.power && l.c0) {  // the table is one chain of products: one lane runs it, everyone multiplies
            if (k0 == 0) {
                V p = E::one();
                for (unsigned i = 0; i < q.slices; ++i) {
                    E::st(buf0, pad, i, p);
                    p = E::mul(p, l.m);
                }
            }
            lds_barrier();
            for (unsigned k = k0; k < q.n; k += nt)
                E::st(l.dst, rp, (size_t)k * q.rel, k < q.slices ? E::mul(E::ld(l.src, fp, (size_t)k * q.xslice), E::ld(buf0, pad, k)) : E::zero());
            lds_barrier();  // (the next line writes the buffer)
            continue;
        }
        const unsigned steps = q.slices - 1;
        unsigned len = q.slen;
        for (unsigned k = k0; k < q.slen; k += nt)
            E::st(buf0, pad, k, E::add(E::zero(), E::ld(l.src, fp, (size_t)(q.slices - 1) * q.xslice + (size_t)k * q.xel)));
        // one-coefficient slices: lane u of the first wave holds the slice of step 64 * b + u, the batch b + 1 is in flight
        const bool single = q.slen == 1;
        V bat = E::zero(), batn = E::zero();
        if (single && wave0 && k0 < steps) batn = E::ld(l.src, fp, (size_t)(steps - 1 - k0) * q.xslice);
        lds_barrier();
        for (unsigned s = 0; s < steps; ++s) {
            const unsigned i = steps - 1 - s;  // the slice this step adds
            const double* src_l = (s & 1u) ? buf1 : buf0;
            double* dst_l = (s & 1u) ? buf0 : buf1;
            const unsigned keep = len + 1 < q.n ? len + 1 : q.n;
            V sv = E::zero();
            if (single && wave0) {
                if ((s & 63u) == 0) {
                    bat = batn;
                    const unsigned sn = s + 64 + k0;
                    if (sn < steps) batn = E::ld(l.src, fp, (size_t)(steps - 1 - sn) * q.xslice);
                }
                sv = obs_shfl<V>(bat, (int)(s & 63u));
            }
            for (unsigned k = k0; k < keep; k += nt) {
                if (!single && k < q.slen) sv = E::ld(l.src, fp, (size_t)i * q.xslice + (size_t)k * q.xel);
                const V lo = k >= 1 ? E::ld(src_l, pad, k - 1) : E::zero();
                const V cur = k < len ? E::ld(src_l, pad, k) : E::zero();
                V r = lin_step<E>(lo, cur, k, len, l.c, l.m, l.c0);
                if (k < q.slen) r = E::add(r, sv);
                E::st(dst_l, pad, k, r);
            }
            len = keep;
            lds_barrier();
        }
        const double* fin = (steps & 1u) ? buf1 : buf0;
        for (unsigned k = k0; k < q.n; k += nt) E::st(l.dst, rp, (size_t)k * q.rel, k < len ? E::ld(fin, pad, k) : E::zero());
        lds_barrier();  // (the next line's first step writes a buffer)
    }
}

}  // namespace gft
