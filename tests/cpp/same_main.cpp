// Test driver of the EAS SAME decoder's adaptor (fm-radio_amd/host/same_decoder_gpu.hpp): a file of station audio [C][n][2] f32 is copied
// to the device and taken in calls of `step` frames with the given hold_ticks and alarm_mask.  Prints per station its status record as
// hex, its flags and ok bytes, and the new messages as "tick kind text|"; exit status 7 where fmd_same_status_dev's records are not
// fmd_same_get_status's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "same_decoder_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: same_main <audio [C][n][2] f32> <n_channels> <fs> <step> <hold_ticks> <alarm_mask>\n"); return 1; }
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
        fmd_host::SameDecoder_GPU dec(C, fs, step);
        fmd_same_params p = dec.GetParams(0);
        if (p.pull != 16 || p.hold_ticks != 750000u) return 6;
        p.hold_ticks = (unsigned)atoll(argv[5]);
        p.alarm_mask = (unsigned)atoi(argv[6]);
        dec.SetParams(p);
        if (dec.GetParams(C - 1).hold_ticks != p.hold_ticks) return 6;
        dec.Update();
        if (dec.Flags(0) != 0 || !dec.IsOk(C - 1) || !dec.NewMessages(0).empty()) return 6;   // before the first Process
        for (long long a = 0; a < n; a += step) {
            const long long k = n - a < step ? n - a : step;
            dec.Process(static_cast<const float*>(d_in) + a * 2, n, k);
        }
        dec.Update();
        for (int c = 0; c < C; c++) {
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&dec.Status(c));
            for (size_t i = 0; i < sizeof(fmd_same_status); i++) printf("%02x", b[i]);
            printf(" %u %d %d", dec.Flags(c), dec.IsOk(c) ? 1 : 0, dec.AlertOpen(c) ? 1 : 0);
            for (const fmd_same_message& m : dec.NewMessages(c)) printf(" %llu %d %.*s|", m.sync_tick, (int)m.kind, (int)m.len, (const char*)m.bytes);
            printf("\n");
            if (!dec.NewMessages(c).empty()) return 6;                       // handed out once
        }
        if (dec.StatusDev() == nullptr || dec.FlagsDev() == nullptr || dec.OkDev() != dec.FlagsDev() + C || dec.GetTotalChannels() != C || dec.GetSampleRate() != fs) return 6;
        // the device's own records are the ones Update() copied
        std::vector<fmd_same_status> dev((size_t)C);
        if (hipMemcpy(dev.data(), dec.StatusDev(), sizeof(fmd_same_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
        for (int c = 0; c < C; c++)
            if (memcmp(&dev[(size_t)c], &dec.Status(c), sizeof(fmd_same_status)) != 0) return 7;
        p.pull = 129;                                                        // refused
        bool threw = false;
        try { dec.SetParams(p, 0); } catch (const std::exception&) { threw = true; }
        if (!threw) return 6;
        dec.Reset();
        dec.Update();
        if (dec.Status(0).frames != 0 || dec.Status(0).accepted != 0 || dec.Flags(0) == 0xFFu || dec.GetParams(0).hold_ticks != (unsigned)atoll(argv[5])) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
