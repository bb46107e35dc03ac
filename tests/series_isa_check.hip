// ISA check of the batched series (tests/test_series_batch_cpu.py): the form-A mul and div kernels of
// genfer_amd/csrc/gft_series_kernels.hpp, the two with no libm inside, instantiated for plain f64.
#include "../genfer_amd/csrc/gft_series_kernels.hpp"

namespace gft {
template __global__ void k_series_mul_a<EF64>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned,
                                              unsigned, unsigned, SeriesBatch);
template __global__ void k_series_div_a<EF64>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned,
                                              unsigned, unsigned, SeriesBatch);
}  // namespace gft
