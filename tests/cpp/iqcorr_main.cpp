// Test driver of the IQ corrector's adaptor (fm-radio_amd/host/iq_corrector_gpu.hpp): built against the C ABI alone.  It runs the
// host-only solve step on the moments given on the command line and prints the correction; device_path() is what a host with a device
// block does, compiled here so that every method of the adaptor is instantiated.
#include <cstdio>
#include <cstdlib>

#include "iq_corrector_gpu.hpp"

// calibrate on a block of cf32 samples on the device, then correct it in place
[[maybe_unused]] static fmd_iq_correction device_path(float* d_block, const int16_t* d_raw, long long n, void* stream) {
    fmd_host::IqCorrector_GPU corr(n);
    corr.Measure(d_block, n, stream);
    const fmd_iq_correction c = corr.Calibrate();
    corr.Process(d_block, n, d_block, stream);
    corr.ResetMoments();
    corr.Process(d_raw, n, d_block, stream);
    corr.SetCorrection(fmd_host::IqCorrector_GPU::Solve(corr.GetMoments()));
    corr.Reset();
    return corr.GetCorrection().dc_i == 0.0f ? c : corr.GetCorrection();
}

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: iqcorr_main <n> <sum_i> <sum_q> <sum_ii> <sum_qq> <sum_iq>\n"); return 1; }
    const fmd_iq_moments m{atof(argv[1]), atof(argv[2]), atof(argv[3]), atof(argv[4]), atof(argv[5]), atof(argv[6])};
    try {
        const fmd_iq_correction c = fmd_host::IqCorrector_GPU::Solve(m);
        printf("%.9g %.9g %.9g %.9g\n", c.dc_i, c.dc_q, c.w_re, c.w_im);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    return 0;
}
