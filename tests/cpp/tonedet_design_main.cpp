// The audio tone detector's host-only unit (fm-radio_amd/csrc/fmd_tonedet_design.cpp) as a stand-alone program, for a sanitizer build:
// for every (floor_db, share_db of slot 0, fs) given the derived thresholds, printed as hex, and the table, written to
// <dir>/table_<fs>.f64; the parameter checks, and both read-outs over records that touch the ends of their rings.  Prints one line of
// thresholds per set of three arguments, then the default parameters' bytes, then "readout ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "fmd_tonedet_design.h"
#include "fmdemod.h"

static void hex(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) std::printf("%02x", b[i]);
    std::printf("\n");
}

static double num(const char* s) { return std::strcmp(s, "-inf") == 0 ? -std::numeric_limits<double>::infinity() : std::atof(s); }

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    fmd_tonedet_params p;
    fmd::TonedetGate g;
    std::string err;
    for (int a = 2; a + 2 < argc; a += 3) {
        static const double share[8] = {0.0, 0.0, 60.0, 1.0, 2.0, 3.0, 4.0, 5.0};
        const int fs = std::atoi(argv[a + 2]);
        std::memset(&p, 0, sizeof(p));
        fmd_tonedet_default_params(&p);
        p.floor_db = num(argv[a]);
        for (int k = 0; k < 8; k++) p.share_db[k] = share[k];
        p.share_db[0] = num(argv[a + 1]);
        if (fmd::tonedet_gate(&p, fs, &g, &err) != FMD_OK) return 1;
        double t[9] = {g.min_e};
        for (int k = 0; k < 8; k++) t[1 + k] = g.c[k];
        hex(t, sizeof(t));
        std::vector<double> tab(2 * (size_t)fs);                             // exactly [fs][2]: a write past either end is caught
        fmd::tonedet_table(fs, tab.data());
        const std::string path = std::string(argv[1]) + "/table_" + std::to_string(fs) + ".f64";
        FILE* fp = std::fopen(path.c_str(), "wb");
        if (!fp || std::fwrite(tab.data(), sizeof(double), tab.size(), fp) != tab.size() || std::fclose(fp) != 0) return 1;
    }
    std::memset(&p, 0, sizeof(p));
    fmd_tonedet_default_params(&p);
    hex(&p, sizeof(p));
    if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_OK || g.min_e != std::pow(10.0, -5.0) * 3200.0 || g.c[3] != std::pow(10.0, -0.6) || g.alarm_mask != 0u) return 1;
    if (g.freq_hz[3] != 853 || g.freq_hz[7] != 0 || g.raise_intervals[7] != 20 || g.clear_intervals[0] != 5) return 1;
    const fmd_tonedet_params good = p;
    // each bound from outside
    for (double v : {inf, nan}) {
        p = good; p.floor_db = v;
        if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_ERR_ARG || err.empty()) return 1;
    }
    for (int k = 0; k < 8; k++) {
        for (int f : {-1, 16000, 16001, 1 << 30}) {
            p = good; p.freq_hz[k] = f;
            if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_ERR_ARG) return 1;
        }
        for (double v : {-1e-9, 60.5, nan, inf}) {
            p = good; p.share_db[k] = v;
            if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_ERR_ARG) return 1;
        }
        p = good; p.raise_intervals[k] = 0;
        if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_ERR_ARG) return 1;
        p = good; p.clear_intervals[k] = 36001;
        if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_ERR_ARG) return 1;
        p = good; p.raise_intervals[k] = 36000; p.clear_intervals[k] = 1; p.freq_hz[k] = 15999; p.share_db[k] = 60.0;
        if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_OK || g.freq_hz[k] != 15999) return 1;
        p.freq_hz[k] = 1; p.share_db[k] = 0.0;
        if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_OK || g.c[k] != 1.0) return 1;
    }
    p = good; p.alarm_mask = 256u;
    if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_ERR_ARG) return 1;
    p = good; p.alarm_mask = 255u; p.floor_db = -inf;
    if (fmd::tonedet_gate(&p, 32000, &g, &err) != FMD_OK || g.min_e != 0.0 || std::signbit(g.min_e)) return 1;
    if (fmd::tonedet_gate(&good, 32005, &g, &err) != FMD_ERR_ARG || fmd::tonedet_gate(nullptr, 32000, &g, &err) != FMD_ERR_ARG) return 1;
    if (fmd::tonedet_interval(8000) != 800 || fmd::tonedet_interval(48000) != 4800 || fmd::tonedet_interval(44100) != 4410) return 1;
    if (fmd::tonedet_interval(7990) != 0 || fmd::tonedet_interval(48010) != 0 || fmd::tonedet_interval(8005) != 0) return 1;

    std::vector<fmd_tonedet_status> st(1);
    std::memset(st.data(), 0, sizeof(fmd_tonedet_status));
    double v = 0.0;
    if (fmd_tonedet_share_db(&st[0], 32000, 0, 1, &v) != FMD_ERR_STATE || fmd_tonedet_level_db(&st[0], 32000, 7, 1, &v) != FMD_ERR_STATE) return 2;
    if (fmd_tonedet_share_db(&st[0], 32005, 0, 1, &v) != FMD_ERR_ARG || fmd_tonedet_level_db(nullptr, 32000, 0, 1, &v) != FMD_ERR_ARG) return 2;
    if (fmd_tonedet_share_db(&st[0], 32000, 8, 1, &v) != FMD_ERR_ARG || fmd_tonedet_share_db(&st[0], 32000, -1, 1, &v) != FMD_ERR_ARG) return 2;
    if (fmd_tonedet_level_db(&st[0], 32000, 0, 1, nullptr) != FMD_ERR_ARG) return 2;
    // a mid signal of mean square 2e-2 a frame of which slot 7 carries a quarter, every slot of the ring in use and the counter past a
    // multiple of 30
    const double M = 3200.0;
    for (int k = 0; k < 30; k++) { st[0].ring_mm[k] = 2e-2 * M; st[0].ring_pw[7][k] = 0.25 * 2e-2 * M * M / 2.0; }
    st[0].intervals = (1ull << 33) + 29;
    for (int w = 1; w <= 30; w++) {
        if (fmd_tonedet_share_db(&st[0], 32000, 7, w, &v) != FMD_OK || std::fabs(v - 10.0 * std::log10(0.25)) > 1e-9) return 3;
        if (fmd_tonedet_level_db(&st[0], 32000, 7, w, &v) != FMD_OK || std::fabs(v - 10.0 * std::log10(0.5e-2)) > 1e-9) return 3;
        if (fmd_tonedet_share_db(&st[0], 32000, 0, w, &v) != FMD_OK || v != -inf) return 3;
    }
    if (fmd_tonedet_share_db(&st[0], 32000, 7, 31, &v) != FMD_ERR_ARG || fmd_tonedet_share_db(&st[0], 32000, 7, 0, &v) != FMD_ERR_ARG) return 4;
    st[0].intervals = 29;
    if (fmd_tonedet_share_db(&st[0], 32000, 7, 30, &v) != FMD_ERR_STATE || fmd_tonedet_share_db(&st[0], 32000, 7, 29, &v) != FMD_OK) return 5;
    // 0 / 0 comes back as it is
    std::memset(st.data(), 0, sizeof(fmd_tonedet_status));
    st[0].intervals = 1;
    if (fmd_tonedet_share_db(&st[0], 32000, 0, 1, &v) != FMD_OK || v == v) return 6;
    if (fmd_tonedet_level_db(&st[0], 32000, 0, 1, &v) != FMD_OK || v != -inf) return 6;
    std::printf("readout ok\n");
    return 0;
}
