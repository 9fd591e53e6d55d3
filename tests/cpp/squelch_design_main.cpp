// The carrier squelch's host-only unit (fm-radio_amd/csrc/fmd_squelch_design.cpp) as a stand-alone program, for a sanitizer build: the
// threshold at every dB given, the parameter checks, and every read-out over records that touch the ends of their rings.  Prints the
// threshold's bytes in hex, one line per argument, then the default parameters' bytes, then "readout ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "fmd_squelch_design.h"
#include "fmdemod.h"

static void hex(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) std::printf("%02x", b[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        const double t = fmd_squelch_threshold(std::atof(argv[a]));
        hex(&t, sizeof(t));
    }
    fmd_squelch_params p;
    std::memset(&p, 0, sizeof(p));
    fmd_squelch_default_params(&p);
    hex(&p, sizeof(p));
    fmd::SquelchGate g;
    std::string err;
    if (fmd::squelch_gate(&p, 12800, &g, &err) != FMD_OK || g.min_s2 != 0.0 || g.c_open != fmd_squelch_threshold(10.0)) return 1;
    p.min_level_db = 20.0;
    if (fmd::squelch_gate(&p, 12800, &g, &err) != FMD_OK || g.min_s2 != std::pow(10.0, 2.0) * 12800.0) return 1;
    p.close_db = 11.0;
    if (fmd::squelch_gate(&p, 12800, &g, &err) != FMD_ERR_ARG || err.empty()) return 1;
    p.close_db = 7.0; p.mode = 3;
    if (fmd::squelch_gate(&p, 12800, &g, &err) != FMD_ERR_ARG) return 1;
    p.mode = 0; p.open_intervals = 1001;
    if (fmd::squelch_gate(&p, 12800, &g, &err) != FMD_ERR_ARG) return 1;
    p.open_intervals = 1; p.min_level_db = std::numeric_limits<double>::quiet_NaN();
    if (fmd::squelch_gate(&p, 12800, &g, &err) != FMD_ERR_ARG) return 1;
    if (fmd::squelch_interval(256000) != 12800 || fmd::squelch_interval(1024000) != 0 || fmd::squelch_interval(256500) != 0) return 1;

    std::vector<fmd_squelch_status> st(1);
    std::memset(st.data(), 0, sizeof(fmd_squelch_status));
    double v = 0.0, c = 0.0, nz = 0.0;
    if (fmd_squelch_level_db(&st[0], 256000, &v) != FMD_ERR_STATE || fmd_squelch_cnr_db(&st[0], 256000, 1, &v) != FMD_ERR_STATE) return 2;
    if (fmd_squelch_cnr_db(&st[0], 512000, 1, &v) != FMD_ERR_ARG || fmd_squelch_cnr_db(nullptr, 256000, 1, &v) != FMD_ERR_ARG) return 2;
    // a carrier of power 1e4 in noise of power 1e2 per sample, every slot of the ring in use and the counter past a multiple of 20
    const double M = 12800.0, A2 = 1e4, s2 = 1e2;
    for (int k = 0; k < 20; k++) { st[0].ring_s2[k] = (A2 + s2) * M; st[0].ring_s4[k] = (A2 * A2 + 4.0 * A2 * s2 + 2.0 * s2 * s2) * M; }
    st[0].intervals = (1ull << 33) + 19;
    for (int w = 1; w <= 20; w++) {
        if (fmd_squelch_cnr_db(&st[0], 256000, w, &v) != FMD_OK || std::fabs(v - 20.0) > 1e-6) return 3;
        if (fmd_squelch_powers(&st[0], 256000, w, &c, &nz) != FMD_OK || std::fabs(c - A2) > 1e-4 || std::fabs(nz - s2) > 1e-4) return 3;
    }
    if (fmd_squelch_level_db(&st[0], 256000, &v) != FMD_OK || std::fabs(v - 10.0 * std::log10(A2 + s2)) > 1e-9) return 3;
    if (fmd_squelch_cnr_db(&st[0], 256000, 21, &v) != FMD_ERR_ARG || fmd_squelch_cnr_db(&st[0], 256000, 0, &v) != FMD_ERR_ARG) return 4;
    st[0].intervals = 19;
    if (fmd_squelch_cnr_db(&st[0], 256000, 20, &v) != FMD_ERR_STATE || fmd_squelch_cnr_db(&st[0], 256000, 19, &v) != FMD_OK) return 5;
    std::printf("readout ok\n");
    return 0;
}
