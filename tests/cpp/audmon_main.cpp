// Test driver of the audio fault monitor's adaptor (fm-radio_amd/host/audio_monitor_gpu.hpp): a file of station audio [C][n][2] f32 is
// copied to the device and taken in calls of `step` frames, with every detector's run lengths given.  Prints per station its status
// record as hex, its flags and ok bytes and the read-outs; exit status 7 where fmd_audmon_status_dev's records are not
// fmd_audmon_get_status's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "audio_monitor_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: audmon_main <audio [C][n][2] f32> <n_channels> <fs> <step> <raise_intervals> <clear_intervals>\n"); return 1; }
    const int C = atoi(argv[2]), fs = atoi(argv[3]);
    const long long step = atoll(argv[4]);
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
        fmd_host::AudioMonitor_GPU mon(C, fs, step);
        fmd_audmon_params p = mon.GetParams(0);
        for (int k = 0; k < 5; k++) { p.raise_intervals[k] = atoi(argv[5]); p.clear_intervals[k] = atoi(argv[6]); }
        mon.SetParams(p);
        if (mon.GetParams(C - 1).clear_intervals[4] != p.clear_intervals[4]) return 6;
        mon.Update();
        if (mon.Flags(0) != 0 || !mon.IsOk(C - 1)) return 6;                  // before the first Process
        for (long long a = 0; a < n; a += step) {
            const long long k = n - a < step ? n - a : step;
            mon.Process(static_cast<const float*>(d_in) + a * 2, n, k);
        }
        mon.Update();
        for (int c = 0; c < C; c++) {
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&mon.Status(c));
            for (size_t i = 0; i < sizeof(fmd_audmon_status); i++) printf("%02x", b[i]);
            printf(" %u %d %.17g %.17g %.17g %.17g\n", mon.Flags(c), mon.IsOk(c) ? 1 : 0, mon.LevelDb(c, 2, 1), mon.BalanceDb(c, 2), mon.Correlation(c, 30),
                   mon.SideMidDb(c, 1));
        }
        if (mon.StatusDev() == nullptr || mon.FlagsDev() == nullptr || mon.OkDev() != mon.FlagsDev() + C || mon.GetTotalChannels() != C) return 6;
        // the device's own records are the ones Update() copied
        std::vector<fmd_audmon_status> dev((size_t)C);
        if (hipMemcpy(dev.data(), mon.StatusDev(), sizeof(fmd_audmon_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
        for (int c = 0; c < C; c++)
            if (memcmp(&dev[(size_t)c], &mon.Status(c), sizeof(fmd_audmon_status)) != 0) return 7;
        p.antiphase_corr = 1.0;                                              // outside (0, 1): refused
        bool threw = false;
        try { mon.SetParams(p, 0); } catch (const std::exception&) { threw = true; }
        if (!threw) return 6;
        mon.ResetPeaks(0);
        mon.Reset();
        mon.Update();
        if (mon.Status(0).frames != 0 || mon.Correlation(0) == mon.Correlation(0) || mon.GetParams(0).raise_intervals[0] != atoi(argv[5])) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
