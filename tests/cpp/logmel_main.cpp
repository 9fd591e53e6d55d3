// Test driver of the log-mel front end's adaptor (fm-radio_amd/host/log_mel_gpu.hpp): a file of station audio [C][n][2] f32 is copied to
// the device and taken in calls of `step` frames at the geometry given.  After every call it appends each station's completed rows to
// OUT.<c>.f32 (through the host views) and at the end prints per station its status record as hex and the time of its last row; exit
// status 7 where the device's views or records are not the host's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "log_mel_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: logmel_main <audio [C][n][2] f32> <n_channels> <fs> <win> <hop> <n_mels> <step> <out prefix>\n"); return 1; }
    const int C = atoi(argv[2]), fs = atoi(argv[3]);
    const long long step = atoll(argv[7]);
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
        fmd_logmel_config cfg;
        if (fmd_logmel_default_config(fs, &cfg) != FMD_OK) return 4;
        cfg.n_channels = C; cfg.win = atoi(argv[4]); cfg.hop = atoi(argv[5]); cfg.n_mels = atoi(argv[6]); cfg.max_input_frames = step;
        fmd_host::LogMel_GPU mel(cfg);
        if (mel.GetTotalChannels() != C || mel.MaxFrames() != (step + cfg.hop - 1) / cfg.hop || mel.OutStride() != mel.MaxFrames() * cfg.n_mels) return 6;
        mel.Update();
        if (mel.Frames(0) != 0 || mel.Status(C - 1).frames != 0) return 6;                        // before the first Process
        std::vector<FILE*> out;
        for (int c = 0; c < C; c++) out.push_back(fopen((std::string(argv[8]) + "." + std::to_string(c) + ".f32").c_str(), "wb"));
        double last_time = 0.0;
        for (long long a = 0; a < n; a += step) {
            const long long k = n - a < step ? n - a : step;
            mel.Process(static_cast<const float*>(d_in) + a * 2, n, k);
            mel.Update();
            for (int c = 0; c < C; c++) {
                for (int t = 0; t < mel.Frames(c); t++) fwrite(mel.Row(c, t), sizeof(float), (size_t)cfg.n_mels, out[(size_t)c]);
                if (c == 0 && mel.Frames(0) > 0) last_time = mel.FrameTime(0, mel.Frames(0) - 1);
                // the device's view of the station is the host's
                std::vector<float> dev((size_t)mel.Frames(c) * (size_t)cfg.n_mels);
                if (!dev.empty()) {
                    if (hipMemcpy(dev.data(), mel.RowsDev(c), sizeof(float) * dev.size(), hipMemcpyDeviceToHost) != hipSuccess) return 7;
                    if (memcmp(dev.data(), mel.Row(c, 0), sizeof(float) * dev.size()) != 0) return 7;
                }
            }
        }
        for (FILE* f : out) fclose(f);
        std::vector<fmd_logmel_status> dev((size_t)C);
        if (hipMemcpy(dev.data(), mel.StatusDev(), sizeof(fmd_logmel_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
        for (int c = 0; c < C; c++) {
            if (memcmp(&dev[(size_t)c], &mel.Status(c), sizeof(fmd_logmel_status)) != 0) return 7;
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&mel.Status(c));
            for (size_t i = 0; i < sizeof(fmd_logmel_status); i++) printf("%02x", b[i]);
            printf(" %.17g\n", last_time);
        }
        bool threw = false;
        try { mel.Process(static_cast<const float*>(d_in), n, step + 1); } catch (const std::exception&) { threw = true; }   // above max_input_frames
        if (!threw) return 6;
        try { (void)mel.Row(0, mel.Frames(0)); threw = false; } catch (const std::out_of_range&) { threw = true; }
        if (!threw) return 6;
        mel.Reset();
        mel.Update();
        if (mel.Status(0).frames != 0 || mel.Status(0).fill != 0) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
