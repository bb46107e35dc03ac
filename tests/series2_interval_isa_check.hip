// ISA check of the batched bivariate interval series (tests/test_interval_series2_cpu.py): the Interval<F64> instantiations of the
// kernels of genfer_amd/csrc/gft_series2_kernels.hpp, from the header alone (the f64 kernels of the header come along).
#include "../genfer_amd/csrc/gft_series2_kernels.hpp"

namespace gft {
template __global__ void k_series2i_mul<EIv>(const double*, const double*, double*, Series2Dims, SeriesBatch, SeriesPlanes);
template __global__ void k_series2i_rec<EIv, SERIES_DIV>(const double*, const double*, double*, Series2Dims, unsigned, SeriesBatch, SeriesPlanes);
template __global__ void k_series2i_rec<EIv, SERIES_EXP>(const double*, const double*, double*, Series2Dims, unsigned, SeriesBatch, SeriesPlanes);
template __global__ void k_series2i_rec<EIv, SERIES_LOG>(const double*, const double*, double*, Series2Dims, unsigned, SeriesBatch, SeriesPlanes);
template __global__ void k_series2i_compose<EIv, true>(const double*, const double*, double*, Series2Dims, int, SeriesBatch, SeriesPlanes);
template __global__ void k_series2i_compose<EIv, false>(const double*, const double*, double*, Series2Dims, int, SeriesBatch, SeriesPlanes);
// the device library's exp / log as the seed == NULL path of exp / log calls them: the FMAs they bring are not the kernels' own
template <bool LOG>
__global__ void k_seed2_probe(const double* x, double* r) {
    const Iv v = LOG ? EIv::log(Iv{x[0], x[1]}) : EIv::exp(Iv{x[0], x[1]});
    r[0] = v.lo;
    r[1] = v.hi;
}
template __global__ void k_seed2_probe<false>(const double*, double*);
template __global__ void k_seed2_probe<true>(const double*, double*);
}  // namespace gft
