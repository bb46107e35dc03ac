// ISA check of the batched compose (tests/test_series_compose_cpu.py): the form-A and form-B kernels of
// genfer_amd/csrc/gft_series_kernels.hpp (form B with g in LDS, the form that runs), instantiated for plain f64.
#include "../genfer_amd/csrc/gft_series_kernels.hpp"

namespace gft {
template __global__ void k_series_compose_a<EF64>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned,
                                                  unsigned, unsigned, SeriesBatch);
template __global__ void k_series_compose_b<EF64, true>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t,
                                                        unsigned, SeriesBatch);
}  // namespace gft
