// The kernels of the fused observation chain (gft_series_observe_chain.hip states the layout and the two forms;
// tests/series_observe_chain_isa_check.hip instantiates them from this file alone).  Templates over the element functor: EF64, EIv.
#pragma once
#include <hip/hip_runtime.h>

#include "gft_elem.hpp"
#include "gft_series.hpp"
#include "gft_series_observe_kernels.hpp"  // obs_shfl

namespace gft {

constexpr unsigned OBC_THREADS_A = 256;  // form A: four waves, a line each
constexpr unsigned OBC_THREADS_B = 512;  // form B: the most lanes of a workgroup

// The lines of a call.  An item has `lines` of them (rank 1: one; rank 2: the first min(other axis, degree_p1) rows or columns -- the
// others are cut away by the truncation before they could reach the result); line j of an item starts j * xline elements into it
// and its coefficients are xel elements apart (the result: rline, rel).  `len`: L_0, the stored length on the axis.
struct ObsChain {
    unsigned lines, len, nsteps, degree_p1;
    int discrete;  // x is given: the factor var(v, x) is part of a step
    size_t xline, xel, rline, rel;
};

// One coefficient of one step from D[kv-1] and D[kv] (the derivative's, D[j] = src[j+1] * ff_j).  The shape rules make every step
// full: the line holds d_t + 1 coefficients, so dl == lout == d_t and kv < dl for every kv the step stores.
//   x == 0:  kv == 0 ? +0 : D[kv-1] * 1                      (mul_var alone)
//   else:    (0 + (kv >= 1 ? D[kv-1] * 1 : +0)) + (x == 1 ? D[kv] : x * D[kv])
template <class E>
__device__ __forceinline__ typename E::V obc_var(typename E::V dlo, typename E::V dhi, unsigned kv, typename E::V x, bool x0, bool x1) {
    typedef typename E::V V;
    if (x0) return kv == 0 ? E::zero() : E::mul(dlo, E::one());
    const V a = kv >= 1 ? E::mul(dlo, E::one()) : E::zero();
    const V r = E::add(E::zero(), a);
    return E::add(r, x1 ? dhi : E::mul(x, dhi));
}
// ... and the step's constant: c == 0 gives +0 (the caller keeps the item at +0 from there on), c == 1 nothing, else c * res
template <class E>
__device__ __forceinline__ typename E::V obc_scale(typename E::V r, typename E::V c, bool c0, bool c1) {
    if (c0) return E::zero();
    return c1 ? r : E::mul(c, r);
}

// what a line needs of its item
template <class E>
struct ObcLine {
    typename E::V x;
    bool x0, x1;
    const double *src, *cs;
    double* dst;
};
template <class E>
__device__ __forceinline__ ObcLine<E> obc_line(size_t line, const ObsChain& q, const SeriesBatch& g, const double* a, const double* xs, size_t xp,
                                               const double* cs, double* res) {
    const size_t qi = line / q.lines;
    const unsigned j = (unsigned)(line - qi * q.lines);
    const SeriesOff o = series_offsets(g, (unsigned)qi);
    ObcLine<E> l;
    l.src = a + o.x + (size_t)j * q.xline;
    l.dst = res + o.r + (size_t)j * q.rline;
    l.cs = cs + o.s;
    l.x = E::zero(), l.x0 = false, l.x1 = false;
    if (q.discrete) {
        l.x = E::ld(xs, xp, o.y);
        l.x0 = E::eq(l.x, E::zero()), l.x1 = E::eq(l.x, E::one());
    }
    return l;
}

// Form A: one wave per line of at most 64 coefficients, lane kv owns position kv for the whole chain.  src[kv + 1] comes from the
// next lane and D[kv - 1] from the previous one; no LDS, no barrier.  The lanes at and above d_t carry values nobody reads.
template <class E>
__global__ void __launch_bounds__(OBC_THREADS_A) k_obs_chain_wave(const double* __restrict__ a, size_t ap, const double* __restrict__ xs, size_t xp,
                                                                 const double* __restrict__ cs, size_t cp, double* __restrict__ res, size_t rp,
                                                                 ObsChain q, const double* __restrict__ tab, size_t tp, SeriesBatch g) {
    typedef typename E::V V;
    const unsigned kv = threadIdx.x & 63;
    const size_t total = (size_t)g.items * q.lines, waves = (size_t)gridDim.x * (OBC_THREADS_A / 64);
    const V ffk = kv + 1 < q.len ? E::ld(tab, tp, kv) : E::zero();  // D[kv] = src[kv + 1] * ff[kv]; ff[kv - 1] travels with D[kv - 1]
    // (a wave is one line: its trip count, x and c are uniform, so the cross-lane reads are never divergent)
    for (size_t line = (size_t)blockIdx.x * (OBC_THREADS_A / 64) + (threadIdx.x >> 6); line < total; line += waves) {
        const ObcLine<E> l = obc_line<E>(line, q, g, a, xs, xp, cs, res);
        V cur = kv < q.len ? E::ld(l.src, ap, (size_t)kv * q.xel) : E::zero();
        bool dead = false;
        V cn = E::ld(l.cs, cp, 0);
        for (unsigned t = 0; t < q.nsteps; ++t) {
            const V c = cn;
            if (t + 1 < q.nsteps) cn = E::ld(l.cs, cp, t + 1);  // the next step's constant: its latency runs beside this step
            const bool c0 = E::is_zero(c), c1 = E::eq(c, E::one());
            dead = dead || c0;
            const V d = E::mul(obs_shfl<V>(cur, (int)((kv + 1) & 63)), ffk);
            V r = d;
            if (q.discrete) r = obc_var<E>(obs_shfl<V>(d, (int)((kv + 63) & 63)), d, kv, l.x, l.x0, l.x1);
            cur = obc_scale<E>(r, c, c0, c1);
        }
        if (dead) cur = E::zero();
        if (kv < q.degree_p1) E::st(l.dst, rp, (size_t)kv * q.rel, cur);
    }
}

// Form B: one workgroup per line, two line buffers of `pad` elements in LDS taking turns (step t reads what step t - 1 wrote, the
// first step reads the operand, the last one writes the result), an LDS-only barrier between the steps.
template <class E>
__global__ void __launch_bounds__(OBC_THREADS_B) k_obs_chain_lds(const double* __restrict__ a, size_t ap, const double* __restrict__ xs, size_t xp,
                                                                const double* __restrict__ cs, size_t cp, double* __restrict__ res, size_t rp,
                                                                ObsChain q, const double* __restrict__ tab, size_t tp, SeriesBatch g, unsigned pad) {
    typedef typename E::V V;
    extern __shared__ double obc_lds[];
    const size_t total = (size_t)g.items * q.lines;
    // the factors of this thread's first position are the same in every step: read once (indices < len - 1)
    const unsigned k0 = threadIdx.x, ntab = q.len - 1;
    const V tab_lo = (k0 >= 1 && k0 - 1 < ntab) ? E::ld(tab, tp, k0 - 1) : E::zero();
    const V tab_hi = k0 < ntab ? E::ld(tab, tp, k0) : E::zero();
    for (size_t line = blockIdx.x; line < total; line += gridDim.x) {
        const ObcLine<E> l = obc_line<E>(line, q, g, a, xs, xp, cs, res);
        bool dead = false;
        // one step; `src(j)` reads coefficient j of the line the step starts from.  The first step (the operand, global memory) and
        // the later ones (LDS) are two instances, so that neither read becomes a flat one
        auto step = [&](unsigned t, auto src) {
            const unsigned dt = q.degree_p1 + (q.nsteps - 1 - t);
            const bool last = t + 1 == q.nsteps;
            double* dst_l = obc_lds + (size_t)(t & 1u) * E::W * pad;
            const V c = E::ld(l.cs, cp, t);
            const bool c0 = E::is_zero(c), c1 = E::eq(c, E::one());
            dead = dead || c0;
            for (unsigned kv = k0; kv < dt; kv += blockDim.x) {
                const bool mine = kv == k0;
                const V d = E::mul(src(kv + 1), mine ? tab_hi : E::ld(tab, tp, kv));
                V r = d;
                if (q.discrete) {
                    const V dlo = kv >= 1 ? E::mul(src(kv), mine ? tab_lo : E::ld(tab, tp, kv - 1)) : E::zero();
                    r = obc_var<E>(dlo, d, kv, l.x, l.x0, l.x1);
                }
                r = obc_scale<E>(r, c, c0, c1);
                if (!last) E::st(dst_l, pad, kv, r);
                else E::st(l.dst, rp, (size_t)kv * q.rel, dead ? E::zero() : r);
            }
            lds_barrier();  // the line passes through LDS only (behind the last step: the next line's first step writes a buffer)
        };
        step(0u, [&](unsigned j) -> V { return E::ld(l.src, ap, (size_t)j * q.xel); });
        for (unsigned t = 1; t < q.nsteps; ++t) {
            const double* src_l = obc_lds + (size_t)((t + 1) & 1u) * E::W * pad;  // what step t - 1 wrote
            step(t, [&](unsigned j) -> V { return E::ld(src_l, pad, j); });
        }
    }
}

}  // namespace gft
