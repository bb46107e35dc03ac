// ISA check of the batched interval series (tests/test_interval_series_cpu.py): the kernels of
// genfer_amd/csrc/gft_series_kernels.hpp instantiated for Interval<F64> (EIv) from that file alone -- the four form-A kernels,
// mul form B, and compose form B with g in LDS (the form that runs).  The two probes at the end hold nothing but the device
// library's exp / log as the seed == NULL path of the exp / log kernels calls them: the test counts their FMAs, the only ones
// the exp / log kernels may have besides those of the IEEE division sequence.
#include "../genfer_amd/csrc/gft_series_kernels.hpp"

namespace gft {
template __global__ void k_series_mul_a<EIv>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned, unsigned,
                                             unsigned, SeriesBatch);
template __global__ void k_series_div_a<EIv>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned, unsigned,
                                             unsigned, SeriesBatch);
template __global__ void k_series_explog_a<EIv, false>(const double*, size_t, unsigned, const double*, size_t, double*, size_t, unsigned, unsigned,
                                                       unsigned, SeriesBatch);
template __global__ void k_series_explog_a<EIv, true>(const double*, size_t, unsigned, const double*, size_t, double*, size_t, unsigned, unsigned,
                                                      unsigned, SeriesBatch);
template __global__ void k_series_compose_a<EIv>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned,
                                                 unsigned, unsigned, SeriesBatch);
template __global__ void k_series_mul_b<EIv>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned, SeriesBatch);
template __global__ void k_series_compose_b<EIv, true>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t,
                                                       unsigned, SeriesBatch);

template <bool LOG>
__global__ void k_seed_probe(const double* x, double* r) {
    const EIv::V v = EIv::ld(x, 64, threadIdx.x);
    EIv::st(r, 64, threadIdx.x, LOG ? EIv::log(v) : EIv::exp(v));
}
template __global__ void k_seed_probe<false>(const double*, double*);
template __global__ void k_seed_probe<true>(const double*, double*);
}  // namespace gft
