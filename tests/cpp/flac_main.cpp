// Test driver of the FLAC recorder (fm-radio_amd/host/flac_recorder_gpu.hpp): a file of station audio [C][n][2] f32 is copied to the
// device and taken in calls of `step` frames; station 0's stream is ended once on the way, after `cut` frames (rounded up to a call).
// Station c's recording goes to <dir>/station_<c>_<stream>.flac.  Prints per station its status record after Close as hex and the
// streams it ended; exit status 7 where fmd_flac_status_dev's records are not fmd_flac_get_status's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "flac_recorder_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: flac_main <audio [C][n][2] f32> <n_channels> <fs> <block_frames> <step> <cut> <dir>\n"); return 1; }
    const int C = atoi(argv[2]), fs = atoi(argv[3]), S = atoi(argv[4]);
    const long long step = atoll(argv[5]), cut = atoll(argv[6]);
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    fseek(fp, 0, SEEK_END); const long bytes = ftell(fp); fseek(fp, 0, SEEK_SET);
    std::vector<unsigned char> cap((size_t)bytes);
    if (fread(cap.data(), 1, cap.size(), fp) != cap.size()) return 2;
    fclose(fp);
    const long long n = (long long)(cap.size() / 8 / (size_t)C);
    void* d_in = nullptr;
    if (hipMalloc(&d_in, cap.size()) != hipSuccess || hipMemcpy(d_in, cap.data(), cap.size(), hipMemcpyHostToDevice) != hipSuccess) return 3;
    std::vector<std::string> stems;
    for (int c = 0; c < C; c++) stems.push_back(std::string(argv[7]) + "/station_" + std::to_string(c));
    try {
        {
            fmd_host::FlacRecorder_GPU rec(stems, fs, step, S);
            if (rec.GetTotalChannels() != C || rec.GetBlockFrames() != (S ? S : 4096)) return 6;
            bool ended = false;
            for (long long a = 0; a < n; a += step) {
                const long long k = n - a < step ? n - a : step;
                rec.Process(static_cast<const float*>(d_in) + a * 2, n, k);
                if (!ended && a + k >= cut) { rec.EndStream(0); ended = true; }
            }
            rec.Update();
            // the device's own records are the ones Update() copied
            std::vector<fmd_flac_status> dev((size_t)C);
            if (rec.StatusDev() == nullptr || hipMemcpy(dev.data(), rec.StatusDev(), sizeof(fmd_flac_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
            for (int c = 0; c < C; c++)
                if (memcmp(&dev[(size_t)c], &rec.Status(c), sizeof(fmd_flac_status)) != 0) return 7;
            rec.Close();
            rec.Close();                                                     // safe to repeat
            for (int c = 0; c < C; c++) {
                const unsigned char* b = reinterpret_cast<const unsigned char*>(&rec.Status(c));
                for (size_t i = 0; i < sizeof(fmd_flac_status); i++) printf("%02x", b[i]);
                printf(" %u\n", rec.StreamIndex(c));
            }
            bool threw = false;
            try { rec.Process(static_cast<const float*>(d_in), n, 1); } catch (const std::exception&) { threw = true; }
            if (!threw) return 6;
        }
        // a second recorder left to its destructor: the file is complete all the same
        {
            std::vector<std::string> one{std::string(argv[7]) + "/left_open"};
            fmd_host::FlacRecorder_GPU rec(one, fs, step, S);
            rec.Process(static_cast<const float*>(d_in), n, n < step ? n : step);
        }
        bool threw = false;
        try { fmd_host::FlacRecorder_GPU bad(stems, fs, step, 100); } catch (const std::exception&) { threw = true; }
        if (!threw) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
