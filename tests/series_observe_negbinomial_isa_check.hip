// ISA check of the fused negative-binomial observation and the Lah row (tests/test_series_observe_negbinomial_cpu.py): the kernels of
// genfer_amd/csrc/gft_series_observe_negbinomial_kernels.hpp, instantiated for F64 and Interval<F64> from that file alone.
#include "../genfer_amd/csrc/gft_series_observe_negbinomial_kernels.hpp"

namespace gft {
#define ONB_INSTANCES(E)                                                                                                                     \
    template __global__ void k_obs_negbin_wave<E>(const double*, size_t, const double*, size_t, const double*, ObsNegbinP, const double*,   \
                                                  size_t, double*, size_t, ObsNegbin, const double*, size_t, SeriesBatch);                   \
    template __global__ void k_obs_negbin_lds<E>(const double*, size_t, const double*, size_t, const double*, ObsNegbinP, const double*,    \
                                                 size_t, double*, size_t, ObsNegbin, const double*, size_t, SeriesBatch, unsigned);          \
    template __global__ void k_lah_row_wave<E>(const double*, size_t, double*, size_t, unsigned, SeriesBatch);                              \
    template __global__ void k_lah_row_lds<E>(const double*, size_t, double*, size_t, unsigned, SeriesBatch, unsigned);
ONB_INSTANCES(EF64)
ONB_INSTANCES(EIv)
}  // namespace gft
