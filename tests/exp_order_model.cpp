// An ordered model of the rank-2 exp recurrence (mt:1271-1300 over mt:971-982), for tests/_exp_order_model.py.
//
//   res[0]  = row0                                                      (a 1-d exp: the caller's)
//   res[k0] = ( sum_{j0} mul_1d(j0 * x[j0], res[k0 - j0]) ) / k0         k0 = 1 .. n0 - 1,  j0 in 1 .. min(k0, xn0 - 1)
//
// with j0 ascending (the reference's order) or descending (the order in which the source rows become available: what
// k_div_wavefront / k_div_wavefront_q / k_rows_wavefront do under `rev`, gft_div2d.hip).  Every row product is formed
// from +0.0 over ascending i, the row products are added to a sum that starts at +0.0, one at a time.  Each multiply,
// add and divide is one rounded binary64 operation: build with -ffp-contract=off and without -ffast-math.  Only the
// terms inside the bounds (i < xnr, i <= c, c - i < nr) are added, whatever the data.
#include <cstddef>
#include <vector>

#include "gft_wavefront_plan.hpp"

extern "C" int exp_order_model(const double* x, unsigned xn0, unsigned xnr, const double* row0, unsigned n0, unsigned nr, int descending,
                               double* res) {
    if (n0 == 0 || nr == 0 || xn0 == 0 || xnr == 0) return 1;
    for (unsigned c = 0; c < nr; ++c) res[c] = row0[c];
    std::vector<double> S(nr), P(nr), a(xnr);
    for (unsigned k0 = 1; k0 < n0; ++k0) {
        for (unsigned c = 0; c < nr; ++c) S[c] = 0.0;
        const unsigned cnt = k0 < xn0 - 1 ? k0 : xn0 - 1;
        for (unsigned t = 0; t < cnt; ++t) {
            const unsigned j0 = descending ? cnt - t : 1 + t;
            const double* b = res + (size_t)(k0 - j0) * nr;
            for (unsigned i = 0; i < xnr; ++i) a[i] = x[(size_t)j0 * xnr + i] * (double)j0;
            for (unsigned c = 0; c < nr; ++c) P[c] = 0.0;
            // (i outside, c inside: every P[c] still receives its terms in ascending i)
            for (unsigned i = 0; i < xnr && i < nr; ++i)
                for (unsigned c = i; c < nr; ++c) P[c] = P[c] + a[i] * b[c - i];
            for (unsigned c = 0; c < nr; ++c) S[c] = S[c] + P[c];
        }
        for (unsigned c = 0; c < nr; ++c) res[(size_t)k0 * nr + c] = S[c] / (double)k0;
    }
    return 0;
}

// Source rows per batch of the f64 kernels (DwfCfg<E>::NW of gft_div2d.hip takes it from the same header).
extern "C" unsigned exp_batch_rows() { return gft::WF_NW_F64; }

// What plan_wavefront selects for exp of x[xn0, xnr] at the result extents (n0, nr): the WfFamily, plus 16 if the family's
// launch arguments — the `rev` its kernels read, not the plan's summary field — carry `rev` (so that the case table's family
// labels are checked against the planner, not against a reading of it).
extern "C" int exp_plan_family(unsigned n0, unsigned nr, unsigned xn0, unsigned xnr, int arrival_order) {
    const size_t z[2] = {n0, nr}, x[2] = {xn0, xnr};
    const gft::WfPlan p = gft::plan_wavefront(gft::WF_EXP, 1, 2, z, x, x, arrival_order != 0);
    const int rev = p.family == gft::WF_ROWS_2D ? p.rows.rev : p.family == gft::WF_NONE ? 0 : p.row.rev;
    return (int)p.family + 16 * (rev != 0);
}
