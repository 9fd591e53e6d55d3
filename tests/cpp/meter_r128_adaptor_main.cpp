// Test driver of the loudness meter's adaptor with both features on (fm-radio_amd/host/loudness_meter_gpu.hpp): a file of audio
// [C][n][2] f32 is copied to the device and metered in calls of `frames_per_call`; per station one line is printed: the 280-byte status
// record and the 24-byte r128 record as hex, the range histogram's total, the loudness range, its two percentiles and the true peak of L
// in dBTP.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "loudness_meter_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: meter_r128_adaptor_main <audio.f32 [C][n][2]> <n_channels> <fs> <frames_per_call>\n"); return 1; }
    const int C = atoi(argv[2]), fs = atoi(argv[3]);
    const long long per = atoll(argv[4]);
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    fseek(fp, 0, SEEK_END); const long bytes = ftell(fp); fseek(fp, 0, SEEK_SET);
    std::vector<float> x((size_t)bytes / 4);
    if (fread(x.data(), 4, x.size(), fp) != x.size()) return 2;
    fclose(fp);
    const long long n = (long long)(x.size() / 2 / (size_t)C);
    float* d_x = nullptr;
    if (hipMalloc(&d_x, x.size() * 4) != hipSuccess || hipMemcpy(d_x, x.data(), x.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return 3;
    try {
        fmd_host::LoudnessMeter_GPU meter(C, fs, per, -1, FMD_METER_TRUE_PEAK | FMD_METER_RANGE);
        for (long long f = 0; f < n; f += per) meter.Process(d_x + 2 * f, n, n - f < per ? n - f : per);
        meter.Update();
        for (int c = 0; c < C; c++) {
            const unsigned char* p = reinterpret_cast<const unsigned char*>(&meter.Status(c));
            for (size_t i = 0; i < sizeof(fmd_meter_status); i++) printf("%02x", p[i]);
            printf(" ");
            p = reinterpret_cast<const unsigned char*>(&meter.R128(c));
            for (size_t i = 0; i < sizeof(fmd_meter_r128_status); i++) printf("%02x", p[i]);
            unsigned total = 0;
            for (int j = 0; j < 1000; j++) total += meter.RangeHistogram(c)[j];
            double low = 0.0, high = 0.0;
            const double lra = meter.LoudnessRange(c, &low, &high);
            printf(" %u %.17g %.17g %.17g %.17g\n", total, lra, low, high, meter.TruePeakDbtp(c, 0));
        }
        if (meter.R128Dev() == nullptr || meter.Features() != 3u) return 6;
        meter.ResetPeaks();
        meter.Update();
        if (meter.R128(0).tp_hold[0] != 0.0f || meter.R128(0).tp_call[1] != 0.0f) return 6;
        meter.Reset();
        meter.Update();
        if (meter.LoudnessRange(0) == meter.LoudnessRange(0)) return 6;        // NaN again
        fmd_host::LoudnessMeter_GPU plain(C, fs, per);
        plain.Update();
        bool threw = false;
        try { (void)plain.R128(0); } catch (const std::out_of_range&) { threw = true; }
        if (!threw || plain.Features() != 0u) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_x);
    return 0;
}
