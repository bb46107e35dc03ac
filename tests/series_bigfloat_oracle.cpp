// TEST INFRASTRUCTURE ONLY -- the BigFloat counterpart of orci_series_mul_raw for the batched BigFloat series tests: the oracle's raw
// 1-d general product mul_rec<BigFloat> (oracle/taylor_oracle.hpp through tests/bigfloat_oracle.cpp, both included unchanged;
// mt:984-1012 over mul_1d, mt:971-982) on plane-major buffers, accumulated onto a zeroed result -- no dispatcher, none of the
// operator's shortcuts.  The whole orcb_ surface of tests/bigfloat_oracle.cpp (the handle operators, orcb_scalar_op) comes with it.
// Built by the tests with g++ -O2 -std=c++17 -ffp-contract=off -shared.
#include "bigfloat_oracle.cpp"

// x: [2][nx] = (factor, exponent), y: [2][ny], res: [2][n], written whole
extern "C" int orcb_series_mul_raw(const double* x, size_t nx, const double* y, size_t ny, double* res, size_t n) {
    try {
        std::vector<BigFloat> xs(nx), ys(ny), zs(n, BigFloat::zero());
        for (size_t i = 0; i < nx; ++i) xs[i] = Tr<BigFloat>::load_plane(x, nx, i);
        for (size_t i = 0; i < ny; ++i) ys[i] = Tr<BigFloat>::load_plane(y, ny, i);
        const View<const BigFloat> xv{xs.data(), {nx}, {1}}, yv{ys.data(), {ny}, {1}};
        const View<BigFloat> rv{zs.data(), {n}, {1}};
        mul_rec<BigFloat>(xv, yv, rv);
        for (size_t k = 0; k < n; ++k) Tr<BigFloat>::store_plane(zs[k], res, n, k);
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}
