// Device side of the batched bivariate series (gft_series2.hip plans and launches these; f64 only).  One workgroup is one item
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
// Multiply and add are rounded separately (-ffp-contract=off) and no explicit fma is written.
#pragma once
#include <hip/hip_runtime.h>

#include "gft_elem.hpp"
#include "gft_series.hpp"
#include "gft_series_kernels.hpp"  // rec_exp, rec_log: row 0 of exp / log is the univariate loop

namespace gft {

// rows x cols doubles from global rows `rstride` apart into a compact LDS array
__device__ inline void s2_stage(double* lds, const double* src, size_t rstride, unsigned rows, unsigned cols) {
    const unsigned total = rows * cols;
    for (unsigned i = threadIdx.x; i < total; i += blockDim.x) {
        const unsigned r = i / cols, c = i - r * cols;
        lds[i] = src[(size_t)r * rstride + c];
    }
}
// the item's result from its compact LDS array: after a __syncthreads that follows every global load of this workgroup, so the
// result may be an operand itself
__device__ inline void s2_store(double* res, size_t rstride, const double* lds, unsigned rows, unsigned cols) {
    const unsigned total = rows * cols;
    for (unsigned i = threadIdx.x; i < total; i += blockDim.x) {
        const unsigned r = i / cols, c = i - r * cols;
        res[(size_t)r * rstride + c] = lds[i];
    }
}

// ---- mul (mt:984-1012) ------------------------------------------------------------------------------------------------------
// z[k0][k1] = 0 + sum_{j0} (0 + sum_{j1} x[j0][j1] * y[k0-j0][k1-j1]), both ascending over the stored coefficients.
// x has pitch d.nx1; `yp` is the pitch of y: d.ny1 for a staged y, its row stride where it stays in global memory.
__device__ inline double s2_mul_out(const double* xl, const double* yl, const Series2Dims& d, size_t yp, unsigned k0, unsigned k1) {
    const unsigned lo0 = k0 + 1 > d.ny0 ? k0 + 1 - d.ny0 : 0, hi0 = k0 + 1 < d.nx0 ? k0 + 1 : d.nx0;
    const unsigned lo1 = k1 + 1 > d.ny1 ? k1 + 1 - d.ny1 : 0, hi1 = k1 + 1 < d.nx1 ? k1 + 1 : d.nx1;
    double z = 0.0;
    for (unsigned j0 = lo0; j0 < hi0; ++j0) {
        const double* xr = xl + j0 * d.nx1;
        const double* yr = yl + (k0 - j0) * yp + k1;
        double o = 0.0;
#pragma unroll 4
        for (unsigned j1 = lo1; j1 < hi1; ++j1) o = o + xr[j1] * yr[-(int)j1];
        z = z + o;
    }
    return z;
}
// x and y staged compactly.  Thread t owns the outputs t and N - 1 - t of the row-major item, (k0, k1) and (n0-1-k0, n1-1-k1): a
// heavy output with a light one, as mul form B pairs k with n - 1 - k.  Lanes of a wave take consecutive k1, so the x address is
// wave-uniform where the bounds agree and the y addresses are consecutive.
__global__ __launch_bounds__(256) void k_series2_mul(const double* x, const double* y, double* res, Series2Dims d, SeriesBatch g) {
    extern __shared__ double s2_lds[];  // [nx0][nx1] | [ny0][ny1]
    double* xl = s2_lds;
    double* yl = s2_lds + d.nx0 * d.nx1;
    const SeriesOff o = series_offsets(g, blockIdx.x);
    s2_stage(xl, x + o.x, d.xr, d.nx0, d.nx1);
    s2_stage(yl, y + o.y, d.yr, d.ny0, d.ny1);
    __syncthreads();  // (every global load of this workgroup is done: the result may be x or y)
    const unsigned N = d.n0 * d.n1, half = (N + 1) / 2;
    for (unsigned t = threadIdx.x; t < half; t += blockDim.x) {
        const unsigned is[2] = {t, N - 1 - t};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned i = is[h];
            if (h == 1 && i == is[0]) break;  // the middle output of an odd N
            const unsigned k0 = i / d.n1, k1 = i - k0 * d.n1;
            res[o.r + (size_t)k0 * d.rr + k1] = s2_mul_out(xl, yl, d, d.ny1, k0, k1);
        }
    }
}

// ---- compose (subst_var's Horner path, mt:569-579) --------------------------------------------------------------------------------
// res = f(g) with g in the place of variable `var` of f.  The slices of f along that axis are its rows (var 0) or its columns (var 1);
// with S of them and `len` coefficients each:
//   res = 0.0 + slice S-1, stored shape (1, len) / (len, 1);  for i = S-2 .. 0:  res = mul(res, g) at the compact shape
//   L = (min(r0 + ng0 - 1, n0), min(r1 + ng1 - 1, n1)) of sum_shape;  row 0 / column 0 of res += slice i
// One workgroup runs the whole loop of its item (the steps are a dependency chain).  Two result arrays of n0 * n1 doubles take turns
// in LDS, the current one compact at pitch r1; g sits compact behind them (GLDS) or stays in global memory at its row stride (the
// fallback where 2 N + ng0 * ng1 doubles exceed the granted LDS).  Every step is k_series2_mul's pairing on a Series2Dims built for
// the step: a thread owns the outputs t and L0 * L1 - 1 - t, all bounds the same for every item; up to 512 lanes.  The owner of an output on the
// added slice loads f's coefficient before its sums and adds it after them -- with GLDS the only global traffic between steps,
// which meet through LDS alone.  f and g are read completely before the first store: the result may be f or g itself.
template <bool GLDS>
__global__ __launch_bounds__(512) void k_series2_compose(const double* f, const double* g, double* res, Series2Dims d, int var, SeriesBatch b) {
    extern __shared__ double s2_lds[];  // res [n0 * n1] | res [n0 * n1] | (GLDS) g [ng0][ng1]
    const unsigned N = d.n0 * d.n1, tid = threadIdx.x, nt = blockDim.x;
    double* cur = s2_lds;
    double* nxt = s2_lds + N;
    const SeriesOff o = series_offsets(b, blockIdx.x);
    const double* fg = f + o.x;
    const double* gs = g + o.y;
    size_t gp = d.yr;
    if (GLDS) {
        double* gl = s2_lds + 2 * N;
        s2_stage(gl, g + o.y, d.yr, d.ny0, d.ny1);
        gs = gl;
        gp = d.ny1;
    }
    // slice i of f is fg[i * fslice + c * fstep], c < len
    const unsigned slices = var == 0 ? d.nx0 : d.nx1, len = var == 0 ? d.nx1 : d.nx0;
    const size_t fslice = var == 0 ? d.xr : 1, fstep = var == 0 ? 1 : d.xr;
    for (unsigned c = tid; c < len; c += nt) cur[c] = 0.0 + fg[(slices - 1) * fslice + c * fstep];
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
                double fv = 0.0;
                if (added) fv = fi[(var == 0 ? k1 : k0) * fstep];  // in flight during the sums below
                double z = s2_mul_out(cur, gs, s, gp, k0, k1);
                if (added) z = z + fv;
                nxt[idx] = z;
            }
        }
        lds_barrier();
        double* sw = cur;
        cur = nxt;
        nxt = sw;
        r0 = s.n0, r1 = s.n1;
    }
    __syncthreads();  // (every global load of this workgroup is done: the result may be f or g)
    for (unsigned idx = tid; idx < N; idx += nt) {
        const unsigned k0 = idx / d.n1, k1 = idx - k0 * d.n1;
        res[o.r + (size_t)k0 * d.rr + k1] = k0 < r0 && k1 < r1 ? cur[k0 * r1 + k1] : 0.0;
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
template <bool WAVE>
__device__ inline void s2_div1d(double* row, const double* yv, unsigned ny1, unsigned n1, unsigned tid, unsigned P) {
    constexpr unsigned EPT = WAVE ? S2_WAVE_EPT : S2_BLOCK_EPT;
    double cur[EPT];
#pragma unroll
    for (unsigned e = 0; e < EPT; ++e) cur[e] = 0.0;
    const double y0 = yv[0];
    for (unsigned j = 0; j < n1; ++j) {
        const unsigned oe = j / P;
        if (tid == j - oe * P) {
#pragma unroll
            for (unsigned e = 0; e < EPT; ++e)
                if (e == oe) row[j] = (-cur[e] + row[j]) / y0;
        }
        s2_step_sync<WAVE>();
        const double q = row[j];
#pragma unroll
        for (unsigned e = 0; e < EPT; ++e) {
            const unsigned i = tid + e * P;
            if (i < n1 && i > j && i - j < ny1) cur[e] = cur[e] + q * yv[i - j];
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
template <int OP>
__global__ __launch_bounds__(256) void k_series2_rec(const double* x, const double* y, double* res, Series2Dims d, unsigned srows,
                                                     SeriesBatch g) {
    constexpr bool DIV = OP == SERIES_DIV, EXP = OP == SERIES_EXP;
    extern __shared__ double s2_lds[];  // A [a0][a1] | r [n0][n1] | scratch [srows][n1]
    const unsigned a0 = DIV ? d.ny0 : d.nx0, a1 = DIV ? d.ny1 : d.nx1, n1 = d.n1;
    double* al = s2_lds;
    double* rl = al + a0 * a1;
    double* sl = rl + d.n0 * n1;
    const unsigned tid = threadIdx.x, nt = blockDim.x;
    const SeriesOff o = series_offsets(g, blockIdx.x);
    if (DIV) s2_stage(al, y + o.y, d.yr, a0, a1);
    else s2_stage(al, x + o.x, d.xr, a0, a1);
    __syncthreads();
    if (!DIV) {  // row 0: the univariate recurrence, a dependency chain on one lane
        if (tid == 0) {
            const RowLds<EF64> xr{al, 0}, rr{rl, 0};
            const double sd = y ? y[o.s] : (EXP ? EF64::exp(al[0]) : EF64::log(al[0]));
            if (EXP) rec_exp<EF64>(xr, rr, a1, n1, sd);
            else rec_log<EF64>(xr, rr, a1, n1, sd);
        }
        lds_barrier();
    }
    for (unsigned k = DIV ? 0u : 1u; k < d.n0; ++k) {
        unsigned jlo, jhi;  // the terms of row k, ascending
        if (EXP) {
            jlo = 1;
            jhi = a0 < k + 1 ? a0 : k + 1;
        } else {
            jlo = k + 1 > a0 ? k + 1 - a0 : 0;
            if (!DIV && jlo < 1) jlo = 1;
            jhi = k;
        }
        double* rk = rl + k * n1;
        for (unsigned jb = jlo; jb < jhi; jb += srows) {
            const unsigned cnt = jhi - jb < srows ? jhi - jb : srows;
            // pass 1: the row sums of the chunk, one (j, k1) a lane
            for (unsigned idx = tid; idx < cnt * n1; idx += nt) {
                const unsigned jj = idx / n1, k1 = idx - jj * n1, j = jb + jj;
                double s = 0.0;
                if (DIV) {  // mul_1d(r[j], y[k-j]): r[j] has n1 coefficients, y[k-j] has ny1
                    const double* a = rl + j * n1;
                    const double* b = al + (k - j) * a1 + k1;
                    const unsigned lo = k1 + 1 > a1 ? k1 + 1 - a1 : 0;
#pragma unroll 4
                    for (unsigned j1 = lo; j1 <= k1; ++j1) s = s + a[j1] * b[-(int)j1];
                } else {
                    const double fj = (double)j;
                    const unsigned hi = k1 + 1 < a1 ? k1 + 1 : a1;
                    if (EXP) {  // mul_1d(x[j] * j, r[k-j]): x[j] * j is rounded before it meets r
                        const double* a = al + j * a1;
                        const double* b = rl + (k - j) * n1 + k1;
#pragma unroll 4
                        for (unsigned j1 = 0; j1 < hi; ++j1) s = s + (a[j1] * fj) * b[-(int)j1];
                    } else {  // mul_1d(x[k-j], r[j] * j)
                        const double* a = al + (k - j) * a1;
                        const double* b = rl + j * n1 + k1;
#pragma unroll 4
                        for (unsigned j1 = 0; j1 < hi; ++j1) s = s + a[j1] * (b[-(int)j1] * fj);
                    }
                }
                sl[idx] = s;
            }
            lds_barrier();
            // pass 2: the ordered additions; r[k] carries the accumulator from chunk to chunk
            for (unsigned k1 = tid; k1 < n1; k1 += nt) {
                double c = jb == jlo ? 0.0 : rk[k1];
                for (unsigned jj = 0; jj < cnt; ++jj) c = c + sl[jj * n1 + k1];
                rk[k1] = c;
            }
            lds_barrier();
        }
        // the row's own step (a lane meets the k1 it owned in pass 2)
        for (unsigned k1 = tid; k1 < n1; k1 += nt) {
            double c = jlo < jhi ? rk[k1] : 0.0;
            if (EXP) {
                c = c / (double)k;
            } else {
                c = -c;
                if (k < d.nx0 && k1 < d.nx1) c = c + (DIV ? x[o.x + (size_t)k * d.xr + k1] : (double)k * al[k * a1 + k1]);
            }
            rk[k1] = c;
        }
        lds_barrier();
        if (!EXP) {
            if (n1 <= 64 * S2_WAVE_EPT) {
                if (tid < 64) s2_div1d<true>(rk, al, a1, n1, tid, 64);
            } else {
                s2_div1d<false>(rk, al, a1, n1, tid, nt);
            }
            lds_barrier();
            if (!DIV) {
                for (unsigned k1 = tid; k1 < n1; k1 += nt) rk[k1] = rk[k1] / (double)k;
                lds_barrier();
            }
        }
    }
    __syncthreads();  // (every global load of this workgroup is done: the result may be an operand)
    s2_store(res + o.r, d.rr, rl, d.n0, n1);
}

}  // namespace gft
