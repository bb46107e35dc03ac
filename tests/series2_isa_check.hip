// ISA check of the batched bivariate series (tests/test_series2_cpu.py): the four kernels of
// genfer_amd/csrc/gft_series2_kernels.hpp, instantiated from the header alone.
#include "../genfer_amd/csrc/gft_series2_kernels.hpp"

namespace gft {
// (k_series2_mul is no template: including the header defines it)
template __global__ void k_series2_rec<SERIES_DIV>(const double*, const double*, double*, Series2Dims, unsigned, SeriesBatch);
template __global__ void k_series2_rec<SERIES_EXP>(const double*, const double*, double*, Series2Dims, unsigned, SeriesBatch);
template __global__ void k_series2_rec<SERIES_LOG>(const double*, const double*, double*, Series2Dims, unsigned, SeriesBatch);
}  // namespace gft
