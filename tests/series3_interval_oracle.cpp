// TEST INFRASTRUCTURE ONLY -- the rank-3 sibling of tests/series2_interval_oracle.cpp for the batched trivariate interval series tests:
// the oracle's raw general product mul_rec<Interval> (oracle/taylor_oracle.hpp, included unchanged; mt:984-1012 over mul_1d,
// mt:971-982) at rank 3 on plane-major buffers, accumulated onto a zeroed result -- no dispatcher, none of the operator's shortcuts.
// Built by the tests with g++ -O2 -std=c++17 -ffp-contract=off -shared.
#include "../oracle/taylor_oracle.hpp"

using namespace orc;

// x: [2][nx0][nx1][nx2] = (lo, hi), y: [2][ny0][ny1][ny2], res: [2][n0][n1][n2], written whole
extern "C" int orci_series3_mul_raw(const double* x, size_t nx0, size_t nx1, size_t nx2, const double* y, size_t ny0, size_t ny1, size_t ny2,
                                    double* res, size_t n0, size_t n1, size_t n2) {
    try {
        const size_t nx = nx0 * nx1 * nx2, ny = ny0 * ny1 * ny2, n = n0 * n1 * n2;
        std::vector<Interval> xs(nx), ys(ny), zs(n, Interval::zero());
        for (size_t i = 0; i < nx; ++i) xs[i] = Interval(x[i], x[nx + i]);
        for (size_t i = 0; i < ny; ++i) ys[i] = Interval(y[i], y[ny + i]);
        const View<const Interval> xv{xs.data(), {nx0, nx1, nx2}, {nx1 * nx2, nx2, 1}}, yv{ys.data(), {ny0, ny1, ny2}, {ny1 * ny2, ny2, 1}};
        const View<Interval> rv{zs.data(), {n0, n1, n2}, {n1 * n2, n2, 1}};
        mul_rec<Interval>(xv, yv, rv);
        for (size_t k = 0; k < n; ++k) {
            res[k] = zs[k].lo;
            res[n + k] = zs[k].hi;
        }
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}
