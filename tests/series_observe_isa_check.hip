// ISA check of the batched observation ops (tests/test_series_observe_cpu.py): the kernels of
// genfer_amd/csrc/gft_series_observe_kernels.hpp, instantiated for F64 and Interval<F64> from that file alone.
#include "../genfer_amd/csrc/gft_series_observe_kernels.hpp"

namespace gft {
#define OBS_INSTANCES(E)                                                                                                                     \
    template __global__ void k_obs_scale<E, false>(const double*, size_t, size_t, double*, size_t, size_t, unsigned, unsigned, unsigned,    \
                                                   unsigned, int, const double*, size_t, SeriesBatch);                                       \
    template __global__ void k_obs_scale<E, true>(const double*, size_t, size_t, double*, size_t, size_t, unsigned, unsigned, unsigned,     \
                                                  unsigned, int, const double*, size_t, SeriesBatch);                                        \
    template __global__ void k_obs_shift_cols<E>(const double*, size_t, size_t, double*, size_t, size_t, unsigned, unsigned, unsigned,      \
                                                 unsigned, int, SeriesBatch);                                                                \
    template __global__ void k_obs_rows<E, false>(const double*, size_t, double*, size_t, ObsRows, SeriesBatch);                            \
    template __global__ void k_obs_rows<E, true>(const double*, size_t, double*, size_t, ObsRows, SeriesBatch);
OBS_INSTANCES(EF64)
OBS_INSTANCES(EIv)
}  // namespace gft
