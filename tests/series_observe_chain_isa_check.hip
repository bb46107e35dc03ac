// ISA check of the fused observation chain (tests/test_series_observe_chain_cpu.py): the kernels of
// genfer_amd/csrc/gft_series_observe_chain_kernels.hpp, instantiated for F64 and Interval<F64> from that file alone.
#include "../genfer_amd/csrc/gft_series_observe_chain_kernels.hpp"

namespace gft {
#define OBC_INSTANCES(E)                                                                                                                     \
    template __global__ void k_obs_chain_wave<E>(const double*, size_t, const double*, size_t, const double*, size_t, double*, size_t,      \
                                                 ObsChain, const double*, size_t, SeriesBatch);                                              \
    template __global__ void k_obs_chain_lds<E>(const double*, size_t, const double*, size_t, const double*, size_t, double*, size_t,       \
                                                ObsChain, const double*, size_t, SeriesBatch, unsigned);
OBC_INSTANCES(EF64)
OBC_INSTANCES(EIv)
}  // namespace gft
