// pow's step planner of the host-side argument layer (genfer_amd/csrc/gft_series_args.hpp, series_pow_steps) on its own: no HIP, no
// device.  Reads one call per line on stdin (tests/test_series_pow_steps.py writes them) and prints the steps it plans:
//   e  nx0 nx1 nx2  n0 n1 n2          (the exponent, the stored shape of x and the orders, right-aligned)
// ->
//   steps <count>
//   <a> <b> <out>  <sa0> <sa1> <sa2>  <sb0> <sb1> <sb2>  <L0> <L1> <L2>  <last>      (one line per product; slots by name)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../genfer_amd/csrc/gft_series_args.hpp"

int main() {
    static const char* const SLOT[5] = {"unit", "ws0", "ws1", "ws2", "result"};
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        uint64_t e = 0;
        unsigned nx[3], n[3];
        in >> e >> nx[0] >> nx[1] >> nx[2] >> n[0] >> n[1] >> n[2];
        if (!in || e > UINT32_MAX) {
            std::printf("BAD LINE %s\n", line.c_str());
            return 2;
        }
        const gft::SeriesPowSteps p = gft::series_pow_steps((uint32_t)e, nx, n);
        std::printf("steps %d\n", p.count);
        for (int i = 0; i < p.count; ++i) {
            const gft::SeriesPowStep& s = p.step[i];
            std::printf("%s %s %s  %u %u %u  %u %u %u  %u %u %u  %d\n", SLOT[s.a], SLOT[s.b], SLOT[s.out], s.sa[0], s.sa[1], s.sa[2], s.sb[0], s.sb[1],
                        s.sb[2], s.L[0], s.L[1], s.L[2], (int)s.last);
        }
    }
    return 0;
}
