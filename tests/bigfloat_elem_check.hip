// The kernels' BigFloat element (EBig, genfer_amd/csrc/gft_elem.hpp) applied to a list of operand pairs, on the host
// pass or (with --device) in a gfx950 kernel.  tests/test_bigfloat_cpu.py and tests/test_bigfloat_gpu.py compare the
// results bit for bit with the test oracle's BigFloat and the interpreter's (gfh_bigfloat_op).
//
//   bigfloat_elem_check [--device] <in.bin> <out.bin>
// in:  n records of 4 doubles {a.factor, a.exponent, b.factor, b.exponent}
// out: n records of NOPS results of 2 doubles, ops in the order of gfh_bigfloat_op: add, sub, mul, div, neg,
//      normalize(a.factor, a.exponent), 0 + b (add0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../genfer_amd/csrc/gft_elem.hpp"

using namespace gft;

static constexpr int NOPS = 7;

GFT_HD inline void apply(const double* in, double* out, size_t i) {
    const Bf a{in[4 * i], in[4 * i + 1]}, b{in[4 * i + 2], in[4 * i + 3]};
    const Bf r[NOPS] = {EBig::add(a, b), EBig::sub(a, b), EBig::mul(a, b), EBig::div(a, b),
                        EBig::neg(a),    EBig::normalize(a.f, a.e), EBig::add0(b)};
    for (int k = 0; k < NOPS; ++k) {
        out[(NOPS * i + k) * 2] = r[k].f;
        out[(NOPS * i + k) * 2 + 1] = r[k].e;
    }
}

__global__ void apply_kernel(const double* in, double* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) apply(in, out, i);
}

#define CHECK(call)                                                                  \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_));        \
            return 3;                                                                \
        }                                                                            \
    } while (0)

int main(int argc, char** argv) {
    const bool device = argc == 4 && strcmp(argv[1], "--device") == 0;
    if (argc != (device ? 4 : 3)) {
        fprintf(stderr, "usage: %s [--device] in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[argc - 2], "rb");
    if (!f) return 2;
    std::vector<double> in;
    double buf[4];
    while (fread(buf, sizeof(double), 4, f) == 4) in.insert(in.end(), buf, buf + 4);
    fclose(f);
    const size_t n = in.size() / 4;
    std::vector<double> out(n * NOPS * 2);
    if (!device) {
        for (size_t i = 0; i < n; ++i) apply(in.data(), out.data(), i);
    } else if (n) {
        double *din = nullptr, *dout = nullptr;
        CHECK(hipMalloc(&din, in.size() * sizeof(double)));
        CHECK(hipMalloc(&dout, out.size() * sizeof(double)));
        CHECK(hipMemcpy(din, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
        const unsigned block = 256;
        apply_kernel<<<(unsigned)((n + block - 1) / block), block>>>(din, dout, n);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost));
        CHECK(hipFree(din));
        CHECK(hipFree(dout));
    }
    FILE* g = fopen(argv[argc - 1], "wb");
    if (!g) return 2;
    fwrite(out.data(), sizeof(double), out.size(), g);
    fclose(g);
    return 0;
}
