// Test driver of the carrier squelch's adaptor (fm-radio_amd/host/carrier_squelch_gpu.hpp): a file of station baseband [C][n][2], cf32
// or u8, is copied to the device and taken in calls of `step` samples, with the gate's parameters given.  Prints per station its status
// record as hex, its mask byte and the read-outs; exit status 7 where fmd_squelch_status_dev's records are not fmd_squelch_get_status's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "carrier_squelch_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: squelch_main <capture [C][n][2]> <cf32|u8> <n_channels> <fs> <step> <open_intervals> <close_intervals>\n"); return 1; }
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
        fmd_host::CarrierSquelch_GPU sq(C, fs, step);
        fmd_squelch_params p = sq.GetParams(0);
        p.open_intervals = atoi(argv[6]); p.close_intervals = atoi(argv[7]);
        sq.SetParams(p);
        if (sq.GetParams(C - 1).close_intervals != p.close_intervals) return 6;
        for (long long a = 0; a < n; a += step) {
            const long long k = n - a < step ? n - a : step;
            if (u8) sq.Process(static_cast<const uint8_t*>(d_in) + a * 2, n, k);
            else sq.Process(static_cast<const float*>(d_in) + a * 2, n, k);
        }
        sq.Update();
        for (int c = 0; c < C; c++) {
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&sq.Status(c));
            for (size_t i = 0; i < sizeof(fmd_squelch_status); i++) printf("%02x", b[i]);
            printf(" %d %.17g %.17g %.17g\n", sq.IsOpen(c) ? 1 : 0, sq.LevelDb(c), sq.CnrDb(c, 1), sq.CnrDb(c, 20));
        }
        if (sq.StatusDev() == nullptr || sq.MaskDev() == nullptr || sq.GetTotalChannels() != C) return 6;
        // the device's own records are the ones Update() copied
        std::vector<fmd_squelch_status> dev((size_t)C);
        if (hipMemcpy(dev.data(), sq.StatusDev(), sizeof(fmd_squelch_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
        for (int c = 0; c < C; c++)
            if (memcmp(&dev[(size_t)c], &sq.Status(c), sizeof(fmd_squelch_status)) != 0) return 7;
        p.close_db = 11.0;                                                   // above open_db: refused
        bool threw = false;
        try { sq.SetParams(p, 0); } catch (const std::exception&) { threw = true; }
        if (!threw) return 6;
        sq.ResetPeaks(0);
        sq.Reset();
        sq.Update();
        if (sq.Status(0).samples != 0 || sq.CnrDb(0) == sq.CnrDb(0) || sq.GetParams(0).open_intervals != atoi(argv[6])) return 6;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
