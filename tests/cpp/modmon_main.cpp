// Test driver of the modulation monitor's adaptor (fm-radio_amd/host/modulation_monitor_gpu.hpp): a file of station baseband
// [C][n][2], cf32 or u8, is copied to the device and monitored in calls of `step` samples.  Prints per station its status record as
// hex, its histogram's total, and the read-outs; exit status 7 where fmd_modmon_status_dev's records are not fmd_modmon_get_status's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "modulation_monitor_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: modmon_main <capture [C][n][2]> <cf32|u8> <n_channels> <fs> <step>\n"); return 1; }
    const bool u8 = strcmp(argv[2], "u8") == 0;
    const int C = atoi(argv[3]), fs = atoi(argv[4]);
    const long long step = atoll(argv[5]);
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    fseek(fp, 0, SEEK_END); const long bytes = ftell(fp); fseek(fp, 0, SEEK_SET);
    std::vector<unsigned char> cap((size_t)bytes);
    if (fread(cap.data(), 1, cap.size(), fp) != cap.size()) return 2;
    fclose(fp);
    const size_t pair = u8 ? 2 : 8;
    const long long n = (long long)(cap.size() / pair / (size_t)C);
    void* d_in = nullptr;
    if (hipMalloc(&d_in, cap.size()) != hipSuccess || hipMemcpy(d_in, cap.data(), cap.size(), hipMemcpyHostToDevice) != hipSuccess) return 3;
    try {
        fmd_host::ModulationMonitor_GPU mon(C, fs, step);
        for (long long a = 0; a < n; a += step) {
            const long long k = n - a < step ? n - a : step;
            if (u8) mon.Process(static_cast<const uint8_t*>(d_in) + a * 2, n, k);
            else mon.Process(static_cast<const float*>(d_in) + a * 2, n, k);
        }
        mon.Update();
        for (int c = 0; c < C; c++) {
            const unsigned char* p = reinterpret_cast<const unsigned char*>(&mon.Status(c));
            for (size_t i = 0; i < sizeof(fmd_modmon_status); i++) printf("%02x", p[i]);
            unsigned total = 0;
            for (int j = 0; j < 300; j++) total += mon.Histogram(c)[j];
            printf(" %u %.17g %.17g %.17g %.17g %.17g %.17g\n", total, mon.DeviationHz(c), mon.OffsetHz(c), mon.PilotHz(c), mon.MpxPowerDbr(c, 1),
                   mon.Exceedance(c, 75000), mon.PercentileHz(c, 0.5));
        }
        if (mon.StatusDev() == nullptr || mon.GetTotalChannels() != C || mon.Design().M != fs / 20) return 6;
        // the device's own records are the ones Update() copied
        std::vector<fmd_modmon_status> dev((size_t)C);
        if (hipMemcpy(dev.data(), mon.StatusDev(), sizeof(fmd_modmon_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
        for (int c = 0; c < C; c++)
            if (memcmp(&dev[(size_t)c], &mon.Status(c), sizeof(fmd_modmon_status)) != 0) return 7;
        mon.ResetPeaks(0);
        mon.Reset();
        mon.Update();
        if (mon.Status(0).samples != 0 || mon.DeviationHz(0) == mon.DeviationHz(0) || mon.Exceedance(0) == mon.Exceedance(0)) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
