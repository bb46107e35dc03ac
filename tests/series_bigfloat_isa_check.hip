// ISA check of the batched BigFloat series (tests/test_bigfloat_series_cpu.py): the kernels of
// genfer_amd/csrc/gft_series_kernels.hpp instantiated for BigFloat (EBig) from that file alone -- the five form-A kernels,
// mul form B, and compose form B with g in LDS (the form that runs).  The two probes at the end hold nothing but EBig::exp / log
// (the device library's exp2 / log2 and the normalisation) as the seed == NULL path of the exp / log kernels calls them: the test
// counts their FMAs, the only ones the exp / log kernels may have besides those of the IEEE division sequence.
#include "../genfer_amd/csrc/gft_series_kernels.hpp"

namespace gft {
template __global__ void k_series_mul_a<EBig>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned, unsigned,
                                             unsigned, SeriesBatch);
template __global__ void k_series_div_a<EBig>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned, unsigned,
                                             unsigned, SeriesBatch);
template __global__ void k_series_explog_a<EBig, false>(const double*, size_t, unsigned, const double*, size_t, double*, size_t, unsigned, unsigned,
                                                       unsigned, SeriesBatch);
template __global__ void k_series_explog_a<EBig, true>(const double*, size_t, unsigned, const double*, size_t, double*, size_t, unsigned, unsigned,
                                                      unsigned, SeriesBatch);
template __global__ void k_series_compose_a<EBig>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned,
                                                 unsigned, unsigned, SeriesBatch);
template __global__ void k_series_mul_b<EBig>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t, unsigned, SeriesBatch);
template __global__ void k_series_compose_b<EBig, true>(const double*, size_t, unsigned, const double*, size_t, unsigned, double*, size_t,
                                                       unsigned, SeriesBatch);

template <bool LOG>
__global__ void k_seed_probe(const double* x, double* r) {
    const EBig::V v = EBig::ld(x, 64, threadIdx.x);
    EBig::st(r, 64, threadIdx.x, LOG ? EBig::log(v) : EBig::exp(v));
}
template __global__ void k_seed_probe<false>(const double*, double*);
template __global__ void k_seed_probe<true>(const double*, double*);
}  // namespace gft
