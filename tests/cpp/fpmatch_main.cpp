// Test driver of the fingerprint matcher's adaptor (fm-radio_amd/host/fingerprint_matcher_gpu.hpp): a file of station words [C][n] u32
// is copied to the device and taken in calls of `step` words against the catalogue in a second file, whose tracks start at the words
// given.  After every call it appends each station's events to OUT.<c>.ev (through the host views) and at the end prints per station its
// status record as hex and its flags byte; exit status 7 where the device's views, bytes or records are not the host's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fingerprint_matcher_gpu.hpp"

static std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> v;
    FILE* fp = fopen(path, "rb");
    if (!fp) return v;
    fseek(fp, 0, SEEK_END); const long bytes = ftell(fp); fseek(fp, 0, SEEK_SET);
    v.resize((size_t)bytes);
    if (fread(v.data(), 1, v.size(), fp) != v.size()) v.clear();
    fclose(fp);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 12) { fprintf(stderr, "usage: fpmatch_main <words [C][n] u32> <n_channels> <n_bits> <block> <interval> <hold> <step> <catalogue u32> <out prefix> <starts>...\n"); return 1; }
    const int C = atoi(argv[2]), step = atoi(argv[7]);
    const std::vector<unsigned char> cap = slurp(argv[1]), catb = slurp(argv[8]);
    if (cap.empty() || catb.empty()) return 2;
    std::vector<long long> starts;
    for (int a = 10; a < argc; a++) starts.push_back(atoll(argv[a]));
    const int T = (int)starts.size() - 1;
    const int n = (int)(cap.size() / 4 / (size_t)C);
    void* d_in = nullptr;
    if (hipMalloc(&d_in, cap.size()) != hipSuccess || hipMemcpy(d_in, cap.data(), cap.size(), hipMemcpyHostToDevice) != hipSuccess) return 3;
    try {
        fmd_fpmatch_config cfg;
        if (fmd_fpmatch_default_config(&cfg) != FMD_OK) return 4;
        cfg.n_channels = C; cfg.n_bits = atoi(argv[3]); cfg.block = atoi(argv[4]); cfg.interval = atoi(argv[5]); cfg.hold = atoi(argv[6]);
        cfg.max_errs = (int)fmd_fpmatch_max_errs(35, cfg.block, cfg.n_bits);
        cfg.max_words = step; cfg.max_tracks = T; cfg.max_catalogue_words = starts.back();
        fmd_host::FingerprintMatcher_GPU m(cfg);
        if (m.GetTotalChannels() != C || m.MaxEvents() != (step + cfg.interval - 1) / cfg.interval || m.StateBytes() <= 0) return 6;
        m.Update();
        if (m.Events(0) != 0 || m.Status(C - 1).words != 0 || m.Status(C - 1).track != -1 || m.Identified(0)) return 6;   // before the first Process
        bool threw = false;
        try { m.Load(reinterpret_cast<const uint32_t*>(catb.data()), starts.data(), T + 1); } catch (const std::exception&) { threw = true; }   // above max_tracks
        if (!threw) return 6;
        m.Load(reinterpret_cast<const uint32_t*>(catb.data()), starts.data(), T);
        std::vector<FILE*> out;
        for (int c = 0; c < C; c++) out.push_back(fopen((std::string(argv[9]) + "." + std::to_string(c) + ".ev").c_str(), "wb"));
        for (int a = 0; a < n; a += step) {
            const int k = n - a < step ? n - a : step;
            m.Process(static_cast<const uint32_t*>(d_in) + a, n, nullptr, k);
            m.Update();
            std::vector<uint8_t> ok((size_t)C), fl((size_t)C);
            if (hipMemcpy(ok.data(), m.OkDev(), (size_t)C, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(fl.data(), m.FlagsDev(), (size_t)C, hipMemcpyDeviceToHost) != hipSuccess)
                return 7;
            for (int c = 0; c < C; c++) {
                std::vector<fmd_fpmatch_event> host;
                for (int i = 0; i < m.Events(c); i++) host.push_back(m.Event(c, i));
                fwrite(host.data(), sizeof(fmd_fpmatch_event), host.size(), out[(size_t)c]);
                // the device's view of the station is the host's, and its bytes follow the record
                std::vector<fmd_fpmatch_event> dev(host.size());
                if (!dev.empty()) {
                    if (hipMemcpy(dev.data(), m.EventsDev(c), sizeof(fmd_fpmatch_event) * dev.size(), hipMemcpyDeviceToHost) != hipSuccess) return 7;
                    if (memcmp(dev.data(), host.data(), sizeof(fmd_fpmatch_event) * dev.size()) != 0) return 7;
                }
                if (ok[(size_t)c] != (m.Status(c).track >= 0 ? 1 : 0) || fl[(size_t)c] != m.Status(c).flags || m.Identified(c) != (ok[(size_t)c] != 0)) return 7;
            }
        }
        for (FILE* o : out) fclose(o);
        std::vector<fmd_fpmatch_status> dev((size_t)C);
        if (hipMemcpy(dev.data(), m.StatusDev(), sizeof(fmd_fpmatch_status) * (size_t)C, hipMemcpyDeviceToHost) != hipSuccess) return 7;
        for (int c = 0; c < C; c++) {
            if (memcmp(&dev[(size_t)c], &m.Status(c), sizeof(fmd_fpmatch_status)) != 0) return 7;
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&m.Status(c));
            for (size_t i = 0; i < sizeof(fmd_fpmatch_status); i++) printf("%02x", b[i]);
            printf(" %d\n", m.Identified(c) ? 1 : 0);
        }
        if (m.BitErrorRate((unsigned)cfg.block * (unsigned)cfg.n_bits / 2u) != 0.5) return 6;
        threw = false;
        try { m.Process(static_cast<const uint32_t*>(d_in), n, nullptr, step + 1); } catch (const std::exception&) { threw = true; }   // above max_words
        if (!threw) return 6;
        try { (void)m.Event(0, m.Events(0)); threw = false; } catch (const std::out_of_range&) { threw = true; }
        if (!threw) return 6;
        m.Reset();
        m.Update();
        if (m.Status(0).words != 0 || m.Status(0).track != -1 || m.Status(0).fill != 0) return 6;
        m.Load(std::vector<std::vector<uint32_t>>());                                              // empties the catalogue
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
