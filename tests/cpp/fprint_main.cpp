// Test driver of the audio fingerprinter's adaptor (fm-radio_amd/host/audio_fingerprint_gpu.hpp): a file of station audio [C][n][2] f32
// is copied to the device and taken in calls of `step` frames at the geometry given.  After every call it appends each station's
// completed words to OUT.<c>.u32 (through the host views) and at the end prints per station its status record as hex and the time of its
// last word; exit status 7 where the device's views or records are not the host's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "audio_fingerprint_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 11) { fprintf(stderr, "usage: fprint_main <audio [C][n][2] f32> <n_channels> <fs> <hop> <n_sub> <n_bands> <f_min> <f_max> <step> <out prefix>\n"); return 1; }
    const int C = atoi(argv[2]), fs = atoi(argv[3]);
    const long long step = atoll(argv[9]);
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
        fmd_fprint_config cfg;
        if (fmd_fprint_default_config(fs, &cfg) != FMD_OK) return 4;
        cfg.n_channels = C; cfg.hop = atoi(argv[4]); cfg.n_sub = atoi(argv[5]); cfg.n_bands = atoi(argv[6]); cfg.f_min_hz = atof(argv[7]); cfg.f_max_hz = atof(argv[8]);
        cfg.max_input_frames = step;
        fmd_host::AudioFingerprint_GPU f(cfg);
        if (f.GetTotalChannels() != C || f.MaxPrints() != (step + cfg.hop - 1) / cfg.hop || f.BitsPerWord() != cfg.n_bands - 1 || f.StateBytes() <= 0) return 6;
        f.Update();
        if (f.Prints(0) != 0 || f.Status(C - 1).frames != 0) return 6;                            // before the first Process
        std::vector<FILE*> out;
        for (int c = 0; c < C; c++) out.push_back(fopen((std::string(argv[10]) + "." + std::to_string(c) + ".u32").c_str(), "wb"));
        double last_time = 0.0;
        for (long long a = 0; a < n; a += step) {
            const long long k = n - a < step ? n - a : step;
            f.Process(static_cast<const float*>(d_in) + a * 2, n, k);
            f.Update();
            for (int c = 0; c < C; c++) {
                std::vector<uint32_t> host;
                for (int i = 0; i < f.Prints(c); i++) host.push_back(f.Word(c, i));
                fwrite(host.data(), sizeof(uint32_t), host.size(), out[(size_t)c]);
                if (c == 0 && f.Prints(0) > 0) last_time = f.WordTime(0, f.Prints(0) - 1);
                // the device's view of the station is the host's
                std::vector<uint32_t> dev(host.size());
                if (!dev.empty()) {
                    if (hipMemcpy(dev.data(), f.WordsDev(c), sizeof(uint32_t) * dev.size(), hipMemcpyDeviceToHost) != hipSuccess) return 7;
                    if (memcmp(dev.data(), host.data(), sizeof(uint32_t) * dev.size()) != 0) return 7;
                    if (fmd_host::AudioFingerprint_GPU::BitErrorRate(dev.data(), host.data(), dev.size()) != 0.0) return 7;
                }
            }
        }
        for (FILE* o : out) fclose(o);
        std::vector<fmd_fprint_status> dev((size_t)C);
        if (hipMemcpy(dev.data(), f.StatusDev(), sizeof(fmd_fprint_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
        for (int c = 0; c < C; c++) {
            if (memcmp(&dev[(size_t)c], &f.Status(c), sizeof(fmd_fprint_status)) != 0) return 7;
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&f.Status(c));
            for (size_t i = 0; i < sizeof(fmd_fprint_status); i++) printf("%02x", b[i]);
            printf(" %.17g\n", last_time);
        }
        const uint32_t a = 0xF0000000u, z = 0u;
        if (fmd_host::AudioFingerprint_GPU::BitErrorRate(&a, &z, 1) != 0.125 || fmd_host::AudioFingerprint_GPU::BitErrorRate(&a, &z, 1, 8) != 0.5) return 6;
        bool threw = false;
        try { f.Process(static_cast<const float*>(d_in), n, step + 1); } catch (const std::exception&) { threw = true; }   // above max_input_frames
        if (!threw) return 6;
        try { (void)f.Word(0, f.Prints(0)); threw = false; } catch (const std::out_of_range&) { threw = true; }
        if (!threw) return 6;
        f.Reset();
        f.Update();
        if (f.Status(0).frames != 0 || f.Status(0).fill != 0) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
