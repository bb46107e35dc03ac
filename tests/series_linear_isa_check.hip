// ISA check of the batched affine substitutions (tests/test_series_linear_cpu.py): the kernels of
// genfer_amd/csrc/gft_series_linear_kernels.hpp, instantiated for F64 and Interval<F64> from that file alone.
#include "../genfer_amd/csrc/gft_series_linear_kernels.hpp"

namespace gft {
#define LIN_INSTANCES(E)                                                                                                                     \
    template __global__ void k_lin_mul<E>(const double*, size_t, const double*, size_t, const double*, size_t, double*, size_t, LinCall,    \
                                          SeriesBatch);                                                                                      \
    template __global__ void k_lin_compose_wave<E>(const double*, size_t, const double*, size_t, const double*, size_t, double*, size_t,    \
                                                   LinCall, SeriesBatch);                                                                    \
    template __global__ void k_lin_compose_lds<E>(const double*, size_t, const double*, size_t, const double*, size_t, double*, size_t,     \
                                                  LinCall, SeriesBatch, unsigned);
LIN_INSTANCES(EF64)
LIN_INSTANCES(EIv)
}  // namespace gft
