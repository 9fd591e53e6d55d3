// Test driver of the fingerprint matcher's adaptor with an index (fm-radio_amd/host/fingerprint_matcher_gpu.hpp, the two-argument
// constructor): a file of station words [C][n] u32 is copied to the device and taken in calls of `step` words against the catalogue in a
// second file, whose tracks start at the words given.  After every call it appends each station's events to OUT.<c>.ev (through the host
// views) and at the end prints per station its status record and its index record as hex; exit status 7 where the adaptor's views are
// not the C interface's, 6 where a brute-force adaptor has an index record.
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

static void hex(const void* p, size_t n) {
    for (size_t i = 0; i < n; i++) printf("%02x", static_cast<const unsigned char*>(p)[i]);
}

int main(int argc, char** argv) {
    if (argc < 14) {
        fprintf(stderr, "usage: fpmatch_index_adaptor_main <words [C][n] u32> <n_channels> <n_bits> <block> <interval> <hold> <step> <max_bucket> <follow> <catalogue u32> "
                        "<out prefix> <starts>...\n");
        return 1;
    }
    const int C = atoi(argv[2]), step = atoi(argv[7]);
    const std::vector<unsigned char> cap = slurp(argv[1]), catb = slurp(argv[10]);
    if (cap.empty() || catb.empty()) return 2;
    std::vector<long long> starts;
    for (int a = 12; a < argc; a++) starts.push_back(atoll(argv[a]));
    const int T = (int)starts.size() - 1;
    const int n = (int)(cap.size() / 4 / (size_t)C);
    void* d_in = nullptr;
    if (hipMalloc(&d_in, cap.size()) != hipSuccess || hipMemcpy(d_in, cap.data(), cap.size(), hipMemcpyHostToDevice) != hipSuccess) return 3;
    try {
        fmd_fpmatch_config cfg;
        fmd_fpmatch_index_config idx;
        if (fmd_fpmatch_default_config(&cfg) != FMD_OK || fmd_fpmatch_index_default_config(&idx) != FMD_OK) return 4;
        cfg.n_channels = C; cfg.n_bits = atoi(argv[3]); cfg.block = atoi(argv[4]); cfg.interval = atoi(argv[5]); cfg.hold = atoi(argv[6]);
        cfg.max_errs = (int)fmd_fpmatch_max_errs(35, cfg.block, cfg.n_bits);
        cfg.max_words = step; cfg.max_tracks = T; cfg.max_catalogue_words = starts.back();
        idx.max_bucket = atoi(argv[8]); idx.follow = atoi(argv[9]);
        {
            fmd_host::FingerprintMatcher_GPU brute(cfg);                                          // no index: no index record
            bool threw = false;
            try { (void)brute.IndexStatus(0); } catch (const std::out_of_range&) { threw = true; }
            if (brute.Indexed() || !threw || brute.StateBytes() != fmd_fpmatch_state_bytes(&cfg)) return 6;
        }
        fmd_fpmatch_index_config bad = idx;
        bad.max_bucket = 65;
        bool threw = false;
        try { fmd_host::FingerprintMatcher_GPU refused(cfg, bad); } catch (const std::exception&) { threw = true; }
        if (!threw) return 6;
        fmd_host::FingerprintMatcher_GPU m(cfg, idx);
        if (!m.Indexed() || m.IndexConfig().max_bucket != idx.max_bucket || m.StateBytes() != fmd_fpmatch_index_state_bytes(&cfg, &idx)) return 6;
        m.Update();
        if (m.IndexStatus(C - 1).candidates != 0 || m.IndexStatus(0).empty != 0) return 6;       // before the first Process
        m.Load(reinterpret_cast<const uint32_t*>(catb.data()), starts.data(), T);
        std::vector<FILE*> out;
        for (int c = 0; c < C; c++) out.push_back(fopen((std::string(argv[11]) + "." + std::to_string(c) + ".ev").c_str(), "wb"));
        for (int a = 0; a < n; a += step) {
            const int k = n - a < step ? n - a : step;
            m.Process(static_cast<const uint32_t*>(d_in) + a, n, nullptr, k);
            m.Update();
            for (int c = 0; c < C; c++)
                for (int i = 0; i < m.Events(c); i++) fwrite(&m.Event(c, i), sizeof(fmd_fpmatch_event), 1, out[(size_t)c]);
        }
        for (FILE* o : out) fclose(o);
        for (int c = 0; c < C; c++) {
            hex(&m.Status(c), sizeof(fmd_fpmatch_status));
            printf(" ");
            hex(&m.IndexStatus(c), sizeof(fmd_fpmatch_index_status));
            printf("\n");
        }
        m.Reset();
        m.Update();
        if (m.Status(0).words != 0 || m.IndexStatus(0).candidates != 0 || m.IndexStatus(C - 1).followed != 0) return 7;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    (void)hipFree(d_in);
    return 0;
}
