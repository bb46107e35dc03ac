// The kernels of the fused negative-binomial observation and of the Lah row (gft_series_observe_negbinomial.hip states the layout and
// the forms; tests/series_observe_negbinomial_isa_check.hip instantiates them from this file alone).  Templates over the element
// functor: EF64, EIv.
#pragma once
#include <hip/hip_runtime.h>

#include "gft_elem.hpp"
#include "gft_series.hpp"
#include "gft_series_linear_kernels.hpp"   // lin_step
#include "gft_series_observe_kernels.hpp"  // obs_shfl

namespace gft {

constexpr unsigned ONB_THREADS_A = 256;  // form A: four waves, a line (an item of the Lah row) each
constexpr unsigned ONB_THREADS_B = 512;  // form B: the most lanes of a workgroup
// form B keeps a thread's part of the sum in registers: ceil(degree_p1 / 512) positions, and 3 * degree_p1 <= SERIES_NEGBIN_MAX
template <class E>
constexpr unsigned ONB_OWN = E::W == 2 ? 3 : 6;
static_assert((size_t)6 * ONB_THREADS_B * 3 >= SERIES_NEGBIN_MAX && (size_t)3 * ONB_THREADS_B * 3 >= SERIES_NEGBIN_MAX_IV,
              "a thread of form B owns at most ONB_OWN positions of the sum");

// The lines of a call, as the chain's (ObsChain): an item has `lines` of them, line j starts j * xline elements into it and its
// coefficients are xel elements apart (the result: rline, rel).  `len`: degree_p1 + order, what a line reads of the operand.
// `columns`: the lines are the columns of a rank-2 item with more than one line -- the reference's product then walks the rows, and
// every term passes through mul_1d's own zero before it joins the sum (mt:984-1012).
struct ObsNegbin {
    unsigned lines, len, order, degree_p1;
    int columns;
    size_t xline, xel, rline, rel;
};
// the scalars p: the plane stride and the batch strides over the collapsed axes of the SeriesBatch
struct ObsNegbinP {
    size_t plane;
    size_t st[IMAXD];
};
__device__ inline size_t onb_p_offset(const SeriesBatch& g, const ObsNegbinP& sp, unsigned it) {
    size_t o = 0;
    unsigned q = it;
    for (int a = g.nd - 1; a >= 0; --a) {
        const unsigned e = g.ext[a], nq = q / e;
        o += (size_t)(q - nq * e) * sp.st[a];
        q = nq;
    }
    return o;
}

// what a line needs of its item: c, m of from(p) * var(v, x, d) -- var itself where p is one by value --, the row, the addresses
template <class E>
struct OnbLine {
    typename E::V c, m;
    bool c0, first;  // c is zero by value (mul_linear keeps mul_var alone); the line holds the item's first element
    const double *src, *ls;
    double* dst;
};
template <class E>
__device__ __forceinline__ OnbLine<E> onb_line(size_t line, const ObsNegbin& q, const SeriesBatch& g, const double* a, const double* xs, size_t xp,
                                               const double* pv, const ObsNegbinP& sp, const double* ls, double* res) {
    typedef typename E::V V;
    const size_t qi = line / q.lines;
    const unsigned j = (unsigned)(line - qi * q.lines);
    const SeriesOff o = series_offsets(g, (unsigned)qi);
    OnbLine<E> l;
    l.src = a + o.x + (size_t)j * q.xline;
    l.dst = res + o.r + (size_t)j * q.rline;
    l.ls = ls + o.s;
    l.first = j == 0;
    const V x = E::ld(xs, xp, o.y), p = E::ld(pv, sp.plane, onb_p_offset(g, sp, (unsigned)qi));
    const bool p1 = E::eq(p, E::one());
    l.c = p1 ? x : E::mul(p, x);
    l.m = p1 ? E::one() : E::mul(p, E::one());
    l.c0 = E::is_zero(l.c);
    return l;
}

// the scaling by the row's entry (Mul's constant order c * x; one by value returns the operand) and the accumulation (Add,
// mt:857-881): pass 0 meets the one-coefficient zero, a zero entry makes the term that zero, which touches the first element only
template <class E>
__device__ __forceinline__ typename E::V onb_accumulate(typename E::V sum, typename E::V u, typename E::V li, unsigned pass, bool first) {
    typedef typename E::V V;
    const bool l0 = E::is_zero(li), l1 = E::eq(li, E::one());
    const V v = l1 ? u : E::mul(li, u);
    if (pass == 0) {
        const V s = l0 ? E::zero() : v;
        return first ? E::add(s, E::zero()) : s;
    }
    if (l0) return first ? E::add(sum, E::zero()) : sum;
    return E::add(E::add(E::zero(), sum), v);
}

// Form A: one wave per line of degree_p1 + order <= 64 coefficients; lane j owns D[j], pf[j], sum[j] and P[j] for all passes.  The
// product of pass i reads S[j - t] and P[t] across lanes (ds_bpermute), t descending so that the terms join in series.mul's order
// (ascending index of S); no LDS, no barrier.  The lanes at and above degree_p1 carry values nobody stores.
template <class E>
__global__ void __launch_bounds__(ONB_THREADS_A) k_obs_negbin_wave(const double* __restrict__ a, size_t ap, const double* __restrict__ xs, size_t xp,
                                                                  const double* __restrict__ pv, ObsNegbinP sp, const double* __restrict__ ls, size_t lp,
                                                                  double* __restrict__ res, size_t rp, ObsNegbin q, const double* __restrict__ tab,
                                                                  size_t tp, SeriesBatch g) {
    typedef typename E::V V;
    const unsigned j = threadIdx.x & 63, d = q.degree_p1;
    const size_t total = (size_t)g.items * q.lines, waves = (size_t)gridDim.x * (ONB_THREADS_A / 64);
    const V ffj = j + 1 < q.len ? E::ld(tab, tp, j) : E::zero();  // D_{i+1}[j] = D_i[j + 1] * ff[j]
    // (a wave is one line: its trip counts and scalars are uniform, so the cross-lane reads are never divergent)
    for (size_t line = (size_t)blockIdx.x * (ONB_THREADS_A / 64) + (threadIdx.x >> 6); line < total; line += waves) {
        const OnbLine<E> l = onb_line<E>(line, q, g, a, xs, xp, pv, sp, ls, res);
        V pf = E::one();  // pf[j] = ((one * m) * m) ..., j factors
        {
            V run = E::one();
            for (unsigned t = 1; t < d; ++t) {
                run = E::mul(run, l.m);
                if (t == j) pf = run;
            }
        }
        V D = j < q.len ? E::ld(l.src, ap, (size_t)j * q.xel) : E::zero();
        V P = j == 0 ? l.c : (j == 1 ? l.m : E::zero());  // P_1; P_0 is never multiplied by
        unsigned plen = 2;
        V sum = E::zero();
        V li = E::ld(l.ls, lp, 0);
        for (unsigned i = 0; i <= q.order; ++i) {
            const V lcur = li;
            if (i < q.order) li = E::ld(l.ls, lp, i + 1);  // the next pass's entry: its latency runs beside this pass
            const V S = E::mul(D, pf);
            V U = S;
            if (i == 1) {
                U = lin_step<E>(obs_shfl<V>(S, (int)((j + 63) & 63)), S, j, d, l.c, l.m, l.c0);
            } else if (i >= 2) {
                V acc = E::zero();
                for (unsigned t = plen; t-- > 0;) {
                    const V pt = obs_shfl<V>(P, (int)t), sv = obs_shfl<V>(S, (int)((j - t) & 63));
                    V term = E::mul(sv, pt);
                    if (q.columns) term = E::add(E::zero(), term);
                    if (j >= t) acc = E::add(acc, term);
                }
                U = q.columns ? acc : E::add(E::zero(), acc);
            }
            sum = onb_accumulate<E>(sum, U, lcur, i, l.first && j == 0);
            if (i < q.order) {
                D = E::mul(obs_shfl<V>(D, (int)((j + 1) & 63)), ffj);
                if (i >= 1) {  // P_{i+1} = mul_linear(P_i, c, m) at min(d, len + 1)
                    const unsigned nlen = plen + 1 < d ? plen + 1 : d;
                    const V nxt = lin_step<E>(obs_shfl<V>(P, (int)((j + 63) & 63)), P, j, plen, l.c, l.m, l.c0);
                    P = j < nlen ? nxt : E::zero();
                    plen = nlen;
                }
            }
        }
        if (j < d) E::st(l.dst, rp, (size_t)j * q.rel, sum);
    }
}

// Form B: one workgroup per line.  D (len elements), S and P (degree_p1 each) lie in LDS, planes `pad` doubles apart; a thread keeps
// the sum of its positions j = threadIdx.x + u * blockDim.x in registers.  A pass: S from D; barrier; the product, and P's next
// coefficients, into registers; barrier; P and the derivative written back (the derivative in rounds of blockDim.x positions,
// ascending, a barrier between a round's reads and its writes); barrier.
template <class E>
__global__ void __launch_bounds__(ONB_THREADS_B) k_obs_negbin_lds(const double* __restrict__ a, size_t ap, const double* __restrict__ xs, size_t xp,
                                                                 const double* __restrict__ pv, ObsNegbinP sp, const double* __restrict__ ls, size_t lp,
                                                                 double* __restrict__ res, size_t rp, ObsNegbin q, const double* __restrict__ tab,
                                                                 size_t tp, SeriesBatch g, unsigned pad) {
    typedef typename E::V V;
    extern __shared__ double onb_lds[];
    double* const Dl = onb_lds;
    double* const Sl = onb_lds + q.len;
    double* const Pl = Sl + q.degree_p1;
    const size_t total = (size_t)g.items * q.lines;
    const unsigned k0 = threadIdx.x, nt = blockDim.x, d = q.degree_p1;
    for (size_t line = blockIdx.x; line < total; line += gridDim.x) {
        const OnbLine<E> l = onb_line<E>(line, q, g, a, xs, xp, pv, sp, ls, res);
        constexpr unsigned OWN = ONB_OWN<E>;
        V pf[OWN], sum[OWN];
        {
            V run = E::one();
#pragma unroll
            for (unsigned u = 0; u < OWN; ++u) pf[u] = run, sum[u] = E::zero();
            for (unsigned t = 1; t < d; ++t) {
                run = E::mul(run, l.m);
#pragma unroll
                for (unsigned u = 0; u < OWN; ++u)
                    if (t == k0 + u * nt) pf[u] = run;
            }
        }
        unsigned plen = 2;
        // one pass; `src(j)` reads coefficient j of D_i.  Pass 0 (the operand, global memory) and the later ones (LDS) are two
        // instances, so that neither read becomes a flat one
        auto pass = [&](unsigned i, auto src) {
            const V li = E::ld(l.ls, lp, i);
            const unsigned dlen = q.len - i;  // of D_i
#pragma unroll
            for (unsigned u = 0; u < OWN; ++u) {
                const unsigned j = k0 + u * nt;
                if (j < d) E::st(Sl, pad, j, E::mul(src(j), pf[u]));
            }
            if (i == 0) {  // D_1 straight from the operand (nothing reads D in this pass), and P_1
                for (unsigned j = k0; j + 1 < dlen; j += nt) E::st(Dl, pad, j, E::mul(src(j + 1), E::ld(tab, tp, j)));
                if (k0 == 0) E::st(Pl, pad, 0, l.c), E::st(Pl, pad, 1, l.m);
            }
            lds_barrier();
            V plo[OWN], pcur[OWN];
            const unsigned nlen = plen + 1 < d ? plen + 1 : d;
#pragma unroll
            for (unsigned u = 0; u < OWN; ++u) {
                const unsigned j = k0 + u * nt;
                plo[u] = pcur[u] = E::zero();
                if (j >= d) continue;
                V U = E::ld(Sl, pad, j);
                if (i == 1) {
                    U = lin_step<E>(j >= 1 ? E::ld(Sl, pad, j - 1) : E::zero(), U, j, d, l.c, l.m, l.c0);
                } else if (i >= 2) {
                    V acc = E::zero();
                    for (unsigned k = j + 1 > plen ? j + 1 - plen : 0; k <= j; ++k) {
                        V term = E::mul(E::ld(Sl, pad, k), E::ld(Pl, pad, j - k));
                        if (q.columns) term = E::add(E::zero(), term);
                        acc = E::add(acc, term);
                    }
                    U = q.columns ? acc : E::add(E::zero(), acc);
                }
                sum[u] = onb_accumulate<E>(sum[u], U, li, i, l.first && j == 0);
                if (i >= 1 && i < q.order && j < nlen) {
                    if (j >= 1) plo[u] = E::ld(Pl, pad, j - 1);
                    if (j < plen) pcur[u] = E::ld(Pl, pad, j);
                }
            }
            if (i >= q.order) return;  // the last pass's derivative and power are not needed
            lds_barrier();
            if (i >= 1) {
#pragma unroll
                for (unsigned u = 0; u < OWN; ++u) {
                    const unsigned j = k0 + u * nt;
                    if (j < nlen) E::st(Pl, pad, j, lin_step<E>(plo[u], pcur[u], j, plen, l.c, l.m, l.c0));
                }
                plen = nlen;
                for (unsigned base = 0; base + 1 < dlen; base += nt) {  // D_{i+1}[j] = D_i[j + 1] * ff[j], in place
                    const unsigned j = base + k0;
                    const bool mine = j + 1 < dlen;
                    V v = E::zero();
                    if (mine) v = E::mul(E::ld(Dl, pad, j + 1), E::ld(tab, tp, j));
                    lds_barrier();
                    if (mine) E::st(Dl, pad, j, v);
                }
            }
            lds_barrier();
        };
        pass(0u, [&](unsigned j) -> V { return E::ld(l.src, ap, (size_t)j * q.xel); });
        for (unsigned i = 1; i <= q.order; ++i) pass(i, [&](unsigned j) -> V { return E::ld(Dl, pad, j); });
#pragma unroll
        for (unsigned u = 0; u < OWN; ++u) {
            const unsigned j = k0 + u * nt;
            if (j < d) E::st(l.dst, rp, (size_t)j * q.rel, sum[u]);
        }
        lds_barrier();  // (the next line's first pass writes S, D and P)
    }
}

// ---- the Lah row (generating_function.rs:713-730) ------------------------------------------------------------------------------------
// row_0 = [one]; row_d[i] = ((one - p) / from(d)) * (row_{d-1}[i] * from(d + i - 1) + row_{d-1}[i - 1]), i = 0 .. d, an absent entry
// of row_{d-1} being zero -- multiplied by and added all the same.
template <class E>
__device__ __forceinline__ typename E::V lah_entry(typename E::V q, typename E::V cur, typename E::V lo, unsigned dd, unsigned i) {
    return E::mul(q, E::add(E::mul(cur, E::from_u32(dd + i - 1)), lo));
}

// one wave per item while order + 1 <= 64: lane i owns entry i, the previous entry comes from lane i - 1
template <class E>
__global__ void __launch_bounds__(ONB_THREADS_A) k_lah_row_wave(const double* __restrict__ pv, size_t pp, double* __restrict__ res, size_t rp,
                                                               unsigned order, SeriesBatch g) {
    typedef typename E::V V;
    const unsigned i = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (ONB_THREADS_A / 64);
    for (size_t it = (size_t)blockIdx.x * (ONB_THREADS_A / 64) + (threadIdx.x >> 6); it < g.items; it += waves) {
        const SeriesOff o = series_offsets(g, (unsigned)it);
        const V omp = E::sub(E::one(), E::ld(pv, pp, o.x));
        V cur = i == 0 ? E::one() : E::zero();  // (the entries a row does not have are zero)
        for (unsigned dd = 1; dd <= order; ++dd) {
            const V q = E::div(omp, E::from_u32(dd));
            const V lo = obs_shfl<V>(cur, (int)((i + 63) & 63));
            const V nxt = lah_entry<E>(q, cur, i >= 1 ? lo : E::zero(), dd, i);
            cur = i <= dd ? nxt : E::zero();
        }
        if (i <= order) E::st(res + o.r, rp, i, cur);
    }
}

// longer rows: one workgroup per item, two rows of `pad` elements in LDS taking turns
template <class E>
__global__ void __launch_bounds__(ONB_THREADS_B) k_lah_row_lds(const double* __restrict__ pv, size_t pp, double* __restrict__ res, size_t rp,
                                                              unsigned order, SeriesBatch g, unsigned pad) {
    typedef typename E::V V;
    extern __shared__ double lah_lds[];
    for (size_t it = blockIdx.x; it < g.items; it += gridDim.x) {
        const SeriesOff o = series_offsets(g, (unsigned)it);
        const V omp = E::sub(E::one(), E::ld(pv, pp, o.x));
        if (threadIdx.x == 0) E::st(lah_lds, pad, 0, E::one());
        lds_barrier();
        for (unsigned dd = 1; dd <= order; ++dd) {
            const double* prev = lah_lds + (size_t)((dd + 1) & 1u) * E::W * pad;
            double* next = lah_lds + (size_t)(dd & 1u) * E::W * pad;
            const V q = E::div(omp, E::from_u32(dd));
            for (unsigned i = threadIdx.x; i <= dd; i += blockDim.x)
                E::st(next, pad, i, lah_entry<E>(q, i < dd ? E::ld(prev, pad, i) : E::zero(), i >= 1 ? E::ld(prev, pad, i - 1) : E::zero(), dd, i));
            lds_barrier();
        }
        const double* last = lah_lds + (size_t)(order & 1u) * E::W * pad;
        for (unsigned i = threadIdx.x; i <= order; i += blockDim.x) E::st(res + o.r, rp, i, E::ld(last, pad, i));
        lds_barrier();  // (the next item writes row 0)
    }
}

}  // namespace gft
