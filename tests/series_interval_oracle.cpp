// TEST INFRASTRUCTURE ONLY -- the interval counterpart of orc_mul_raw for the batched interval series tests: the oracle's raw
// 1-d general product mul_rec<Interval> (oracle/taylor_oracle.hpp, included unchanged; mt:984-1012 over mul_1d, mt:971-982) on
// plane-major buffers, accumulated onto a zeroed result -- no dispatcher, none of the operator's shortcuts.  Built by the tests
// with g++ -O2 -std=c++17 -ffp-contract=off -shared.
#include "../oracle/taylor_oracle.hpp"

using namespace orc;

// x: [2][nx] = (lo, hi), y: [2][ny], res: [2][n], written whole
extern "C" int orci_series_mul_raw(const double* x, size_t nx, const double* y, size_t ny, double* res, size_t n) {
    try {
        std::vector<Interval> xs(nx), ys(ny), zs(n, Interval::zero());
        for (size_t i = 0; i < nx; ++i) xs[i] = Interval(x[i], x[nx + i]);
        for (size_t i = 0; i < ny; ++i) ys[i] = Interval(y[i], y[ny + i]);
        const View<const Interval> xv{xs.data(), {nx}, {1}}, yv{ys.data(), {ny}, {1}};
        const View<Interval> rv{zs.data(), {n}, {1}};
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
