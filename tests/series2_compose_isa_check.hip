// ISA check of the batched bivariate compose (tests/test_series2_compose_cpu.py): both instantiations of k_series2_compose of
// genfer_amd/csrc/gft_series2_kernels.hpp (g resident in LDS, g in global memory), instantiated from the header alone.
#include "../genfer_amd/csrc/gft_series2_kernels.hpp"

namespace gft {
template __global__ void k_series2_compose<true>(const double*, const double*, double*, Series2Dims, int, SeriesBatch);
template __global__ void k_series2_compose<false>(const double*, const double*, double*, Series2Dims, int, SeriesBatch);
}  // namespace gft
