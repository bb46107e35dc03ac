// The kernels of the batched observation ops (gft_series_observe.hip states the layout and the roles; tests/series_observe_isa_check.hip
// instantiates them from this file alone).  Templates over the element functor: EF64, EIv.
#pragma once
#include <hip/hip_runtime.h>

#include "gft_elem.hpp"
#include "gft_series.hpp"

namespace gft {

constexpr unsigned OBS_THREADS = 256;

// item and the position inside the item of the linear index `lin` (per = elements per item, < 2^13)
__device__ inline void obs_split(size_t lin, unsigned per, bool narrow, unsigned& it, unsigned& rem) {
    if (narrow) {  // the whole index space fits 32 bits: no 64-bit division
        const unsigned l = (unsigned)lin;
        it = l / per;
        rem = l - it * per;
    } else {
        const size_t q = lin / per;
        it = (unsigned)q;
        rem = (unsigned)(lin - q * per);
    }
}

// out[r][c] = x[r + k0][c + k1] * tab[slice], slice the index along the scaled axis (var 0: r, var 1: c); COPY0 leaves slice 0
// untouched (taylor_expansion_of_coeff).  (m0, m1): the result's shape.
template <class E, bool COPY0>
__global__ void __launch_bounds__(OBS_THREADS) k_obs_scale(const double* __restrict__ x, size_t xp, size_t xr, double* __restrict__ res, size_t rp,
                                                          size_t rr, unsigned m0, unsigned m1, unsigned k0, unsigned k1, int var,
                                                          const double* __restrict__ tab, size_t tp, SeriesBatch g) {
    typedef typename E::V V;
    const unsigned per = m0 * m1;
    const size_t total = (size_t)g.items * per;
    const bool narrow = total <= 0xffffffffull;
    for (size_t lin = blockIdx.x * (size_t)blockDim.x + threadIdx.x; lin < total; lin += (size_t)gridDim.x * blockDim.x) {
        unsigned it, rem;
        obs_split(lin, per, narrow, it, rem);
        const unsigned r = rem / m1, c = rem - r * m1;
        const SeriesOff o = series_offsets(g, it);
        const V v = E::ld(x, xp, o.x + (size_t)(r + k0) * xr + (c + k1));
        const unsigned s = var == 0 ? r : c;
        V out = v;
        if (!COPY0 || s != 0) out = E::mul(v, E::ld(tab, tp, s));
        E::st(res, rp, o.r + (size_t)r * rr + c, out);
    }
}

// shift_down along axis 0, n1 > 1: out[0][c] = x[k][c] + (0.0 + x[0][c] + ... + x[cnt-1][c]) (`whole`: the sum alone, over every
// row), out[r][c] = x[k + r][c] for r >= 1
template <class E>
__global__ void __launch_bounds__(OBS_THREADS) k_obs_shift_cols(const double* __restrict__ x, size_t xp, size_t xr, double* __restrict__ res, size_t rp,
                                                               size_t rr, unsigned m0, unsigned m1, unsigned k, unsigned cnt, int whole,
                                                               SeriesBatch g) {
    typedef typename E::V V;
    const unsigned per = m0 * m1;
    const size_t total = (size_t)g.items * per;
    const bool narrow = total <= 0xffffffffull;
    for (size_t lin = blockIdx.x * (size_t)blockDim.x + threadIdx.x; lin < total; lin += (size_t)gridDim.x * blockDim.x) {
        unsigned it, rem;
        obs_split(lin, per, narrow, it, rem);
        const unsigned r = rem / m1, c = rem - r * m1;
        const SeriesOff o = series_offsets(g, it);
        const double* col = x + o.x + c;
        V out;
        if (r == 0) {
            V acc = E::zero();
            for (unsigned i = 0; i < cnt; ++i) acc = E::add(acc, E::ld(col, xp, (size_t)i * xr));
            out = whole ? acc : E::add(E::ld(col, xp, (size_t)k * xr), acc);
        } else
            out = E::ld(col, xp, (size_t)(k + r) * xr);
        E::st(res, rp, o.r + (size_t)r * rr + c, out);
    }
}

template <class V>
__device__ inline V obs_shfl(V v, int lane);
template <>
__device__ inline double obs_shfl<double>(double v, int lane) {
    return __shfl(v, lane, 64);
}
template <>
__device__ inline Iv obs_shfl<Iv>(Iv v, int lane) {
    return Iv{__shfl(v.lo, lane, 64), __shfl(v.hi, lane, 64)};
}

// The geometry of a row for k_obs_rows: element e of row r of an item is at  r * xrow + (e / inner) * xes + e % inner  (an
// evaluate_all_one item is one "row" of n0 * n1 elements, inner = n1 and xes the row stride; a one-column item summed along axis 0
// has inner = 1 and xes the row stride); the result's element j of row r at  r * rrow + j * res_es.
struct ObsRows {
    unsigned rows;   // per item
    unsigned inner;  // see above; e / inner == 0 for every e when `flat`
    int flat;
    size_t xrow, xes, rrow, res_es;
    unsigned cnt;    // elements 0 .. cnt-1 enter the sum
    unsigned k;      // shift_down: out[0] = x[k] + sum; out[j] = x[k + j], j < m
    unsigned m;      // the result's elements per row (evaluate_all_one: 1)
    int whole;       // out[0] is the sum alone (evaluate_all_one; shift_down with len == k + 1)
};

// eight lanes per row; see the head of the file
template <class E, bool FOLD8>
__global__ void __launch_bounds__(OBS_THREADS) k_obs_rows(const double* __restrict__ x, size_t xp, double* __restrict__ res, size_t rp, ObsRows q,
                                                         SeriesBatch g) {
    typedef typename E::V V;
    const unsigned u = threadIdx.x & 7;
    const int lane = (int)(threadIdx.x & 63), base = lane & ~7;
    const size_t total = (size_t)g.items * q.rows;  // rows in all
    const size_t groups = (size_t)gridDim.x * (blockDim.x >> 3);
    // (every lane of a wave makes the same number of trips: the shuffles below are never divergent)
    const size_t trips = (total + groups - 1) / groups;
    size_t row = (size_t)blockIdx.x * (blockDim.x >> 3) + (threadIdx.x >> 3);
    for (size_t t = 0; t < trips; ++t, row += groups) {
        const bool live = row < total;
        unsigned it = 0, r = 0;
        if (live) {
            const size_t qi = row / q.rows;
            it = (unsigned)qi;
            r = (unsigned)(row - qi * q.rows);
        }
        const SeriesOff o = series_offsets(g, it);
        const double* xrow = x + o.x + (size_t)r * q.xrow;
        auto at = [&](unsigned e) -> size_t {
            if (q.flat) return e;
            const unsigned hi = e / q.inner;
            return (size_t)hi * q.xes + (e - hi * q.inner);
        };
        const unsigned cnt = live ? q.cnt : 0;
        V acc = E::zero();
        unsigned e = 0;
        if (FOLD8) {
            V p = E::zero();
            for (; e + 8 <= cnt; e += 8) p = E::add(p, E::ld(xrow, xp, at(e + u)));
            const V hi4 = obs_shfl<V>(p, base + ((u + 4) & 7));
            const V pair = E::add(p, hi4);  // lanes 0..3: p[u] + p[u+4]
            for (int i = 0; i < 4; ++i) acc = E::add(acc, obs_shfl<V>(pair, base + i));
        } else {
            for (; e + 8 <= cnt; e += 8) {
                const V v = E::ld(xrow, xp, at(e + u));
                for (int i = 0; i < 8; ++i) acc = E::add(acc, obs_shfl<V>(v, base + i));
            }
        }
        {  // the tail, fewer than eight elements, in order
            const unsigned left = cnt - e;
            V v = E::zero();
            if (u < left) v = E::ld(xrow, xp, at(e + u));
            for (unsigned i = 0; i < 7; ++i) {
                const V w = obs_shfl<V>(v, base + (int)i);
                if (i < left) acc = E::add(acc, w);
            }
        }
        if (!live) continue;
        double* rrow = res + o.r + (size_t)r * q.rrow;
        if (u == 0) E::st(rrow, rp, 0, q.whole ? acc : E::add(E::ld(xrow, xp, at(q.k)), acc));
        for (unsigned j = u == 0 ? 8 : u; j < q.m; j += 8) E::st(rrow, rp, (size_t)j * q.res_es, E::ld(xrow, xp, at(q.k + j)));
    }
}

}  // namespace gft
