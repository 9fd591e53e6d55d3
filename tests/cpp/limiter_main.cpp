// Test driver of the limiter's adaptor (fm-radio_amd/host/audio_limiter_gpu.hpp): a file of station audio [C][n][2] f32 is copied to the
// device and taken in calls of `step` frames, station c at gain 0.5 + c; the outputs, the flush's frames behind them, go to <out> as
// [C][n + D][2] f32.  Prints per station its status record as hex; exit status 7 where fmd_limiter_status_dev's records are not
// fmd_limiter_get_status's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "audio_limiter_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: limiter_main <audio [C][n][2] f32> <n_channels> <fs> <lookahead_ms> <release_ms> <step> <out>\n"); return 1; }
    const int C = atoi(argv[2]), fs = atoi(argv[3]);
    const double la = atof(argv[4]), rel = atof(argv[5]);
    const long long step = atoll(argv[6]);
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    fseek(fp, 0, SEEK_END); const long bytes = ftell(fp); fseek(fp, 0, SEEK_SET);
    std::vector<unsigned char> cap((size_t)bytes);
    if (fread(cap.data(), 1, cap.size(), fp) != cap.size()) return 2;
    fclose(fp);
    const long long n = (long long)(cap.size() / 8 / (size_t)C);
    void* d_in = nullptr;
    if (hipMalloc(&d_in, cap.size()) != hipSuccess || hipMemcpy(d_in, cap.data(), cap.size(), hipMemcpyHostToDevice) != hipSuccess) return 3;
    try {
        fmd_host::AudioLimiter_GPU lim(C, fs, step, la, rel);
        const int D = lim.GetLatency();
        if (lim.GetTotalChannels() != C || lim.OutStride() < step || lim.GetGain(0) != 1.0f) return 6;
        for (int c = 0; c < C; c++) lim.SetGain(0.5f + (float)c, c);
        if (lim.GetGain(C - 1) != 0.5f + (float)(C - 1)) return 6;
        std::vector<float> y((size_t)C * (size_t)(n + D) * 2);
        auto collect = [&](const float* d_y, long long at, long long k) {
            if (k > 0 && hipMemcpy2D(y.data() + at * 2, sizeof(float) * 2 * (size_t)(n + D), d_y, sizeof(float) * 2 * (size_t)lim.OutStride(), sizeof(float) * 2 * (size_t)k,
                                     (size_t)C, hipMemcpyDeviceToHost) != hipSuccess)
                throw std::runtime_error("the output's copy failed");
        };
        for (long long a = 0; a < n; a += step) {
            const long long k = n - a < step ? n - a : step;
            collect(lim.Process(static_cast<const float*>(d_in) + a * 2, n, k), a, k);
        }
        collect(lim.Flush(), n, D);
        lim.Update();
        std::vector<fmd_limiter_status> dev((size_t)C);
        if (lim.StatusDev() == nullptr || hipMemcpy(dev.data(), lim.StatusDev(), sizeof(fmd_limiter_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
        for (int c = 0; c < C; c++) {
            if (memcmp(&dev[(size_t)c], &lim.Status(c), sizeof(fmd_limiter_status)) != 0) return 7;
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&lim.Status(c));
            for (size_t i = 0; i < sizeof(fmd_limiter_status); i++) printf("%02x", b[i]);
            printf("\n");
        }
        fp = fopen(argv[7], "wb");
        if (!fp || fwrite(y.data(), sizeof(float), y.size(), fp) != y.size()) return 2;
        fclose(fp);
        bool threw = false;
        try { lim.SetGain(-1.0f); } catch (const std::exception&) { threw = true; }
        if (!threw) return 6;
        threw = false;
        try { fmd_host::AudioLimiter_GPU bad(C, fs, step, 100.0); } catch (const std::exception&) { threw = true; }
        if (!threw) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
