// ISA check of the transposed products (tests/test_series_corr_cpu.py): corr in form A and form B and the transposed Horner loop
// compose_adj (with g in LDS, the form that runs) of genfer_amd/csrc/gft_series_kernels.hpp, instantiated for plain f64.
#include "../genfer_amd/csrc/gft_series_kernels.hpp"

namespace gft {
template __global__ void k_series_corr_a<EF64>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned,
                                               unsigned, unsigned, SeriesBatch);
template __global__ void k_series_corr_b<EF64>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned,
                                               SeriesBatch);
template __global__ void k_series_compose_adj_b<EF64, true>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t,
                                                            unsigned, SeriesBatch);
}  // namespace gft
