// Test driver of the audio tone detector's adaptor (fm-radio_amd/host/tone_detector_gpu.hpp): a file of station audio [C][n][2] f32 is
// copied to the device and taken in calls of `step` frames, with every slot's run lengths given.  Prints per station its status record
// as hex, its flags and ok bytes and the read-outs of slots 0 and 3; exit status 7 where fmd_tonedet_status_dev's records are not
// fmd_tonedet_get_status's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tone_detector_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: tonedet_main <audio [C][n][2] f32> <n_channels> <fs> <step> <raise_intervals> <clear_intervals>\n"); return 1; }
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
        fmd_host::ToneDetector_GPU det(C, fs, step);
        fmd_tonedet_params p = det.GetParams(0);
        for (int k = 0; k < 8; k++) { p.raise_intervals[k] = atoi(argv[5]); p.clear_intervals[k] = atoi(argv[6]); }
        p.alarm_mask = 1u;                                                   // the 1000 Hz slot is an alarm
        det.SetParams(p);
        if (det.GetParams(C - 1).clear_intervals[7] != p.clear_intervals[7]) return 6;
        det.Update();
        if (det.Flags(0) != 0 || !det.IsOk(C - 1) || det.Status(0).freq_hz[3] != 853) return 6;   // before the first Process
        for (long long a = 0; a < n; a += step) {
            const long long k = n - a < step ? n - a : step;
            det.Process(static_cast<const float*>(d_in) + a * 2, n, k);
        }
        det.Update();
        for (int c = 0; c < C; c++) {
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&det.Status(c));
            for (size_t i = 0; i < sizeof(fmd_tonedet_status); i++) printf("%02x", b[i]);
            printf(" %u %d %.17g %.17g %.17g %.17g\n", det.Flags(c), det.IsOk(c) ? 1 : 0, det.ShareDb(c, 0, 1), det.LevelDb(c, 0, 2), det.ShareDb(c, 3, 30),
                   det.LevelDb(c, 3, 1));
        }
        if (det.StatusDev() == nullptr || det.FlagsDev() == nullptr || det.OkDev() != det.FlagsDev() + C || det.GetTotalChannels() != C) return 6;
        // the device's own records are the ones Update() copied
        std::vector<fmd_tonedet_status> dev((size_t)C);
        if (hipMemcpy(dev.data(), det.StatusDev(), sizeof(fmd_tonedet_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
        for (int c = 0; c < C; c++)
            if (memcmp(&dev[(size_t)c], &det.Status(c), sizeof(fmd_tonedet_status)) != 0) return 7;
        p.freq_hz[0] = fs / 2;                                               // not below fs / 2: refused
        bool threw = false;
        try { det.SetParams(p, 0); } catch (const std::exception&) { threw = true; }
        if (!threw) return 6;
        det.Reset();
        det.Update();
        if (det.Status(0).frames != 0 || det.ShareDb(0, 0) == det.ShareDb(0, 0) || det.GetParams(0).raise_intervals[0] != atoi(argv[5])) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
