// The worst case of flog10 (fm-radio_amd/csrc/fmd_logmel_math.h) over EVERY finite float >= FLT_MIN against the host's float64 log10,
// in fp32 ulps of the exact value.  Host only, about a minute on a few cores; the figure goes into DESIGN.md §6n, and
// tests/test_logmel_cpu.py pins it on a subset.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -pthread -Ifm-radio_amd/csrc tools/logmel_flog10_sweep.cpp -o /tmp/flog10_sweep && /tmp/flog10_sweep
//
// With arguments `first last stride` (bit patterns) it sweeps that range only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "fmd_logmel_math.h"

// |y - ref| in ulps of (float)ref's binade (the ulp of a zero reference is that of the smallest normal float)
static double ulp_error(float y, double ref) {
    int e;
    (void)std::frexp(std::fabs(ref) < 1.17549435e-38 ? 1.17549435e-38 : ref, &e);
    return std::fabs((double)y - ref) / std::ldexp(1.0, e - 24);
}

int main(int argc, char** argv) {
    const uint64_t first = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 0x00800000ull;
    const uint64_t last = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 0x7f7fffffull;
    const uint64_t stride = argc > 3 ? std::strtoull(argv[3], nullptr, 0) : 1ull;
    const unsigned T = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<double> worst(T, 0.0);
    std::vector<uint32_t> at(T, 0u);
    std::vector<uint64_t> count(T, 0ull);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < T; t++)
        pool.emplace_back([&, t] {
            for (uint64_t b = first + (uint64_t)t * stride; b <= last; b += (uint64_t)T * stride) {
                const float x = fmd::lm_bits_f32((uint32_t)b);
                const double err = ulp_error(fmd::flog10(x), std::log10((double)x));
                count[t]++;
                if (err > worst[t]) { worst[t] = err; at[t] = (uint32_t)b; }
            }
        });
    for (auto& th : pool) th.join();
    double w = 0.0; uint32_t a = 0; uint64_t n = 0;
    for (unsigned t = 0; t < T; t++) { n += count[t]; if (worst[t] > w) { w = worst[t]; a = at[t]; } }
    std::printf("floats %llu  worst %.4f ulp at 0x%08x (%.9g)\n", (unsigned long long)n, w, a, (double)fmd::lm_bits_f32(a));
    return w <= 8.0 ? 0 : 1;
}
