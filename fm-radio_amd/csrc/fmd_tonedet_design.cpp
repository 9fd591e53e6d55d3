// Built with -ffp-contract=off -fno-fast-math (Makefile): every double operation is the one written, so the table, the thresholds and
// the read-outs are the pure functions that tests/cpp/tonedet_ref.c restates.
#include "fmd_tonedet_design.h"

#include <cmath>
#include <limits>

namespace fmd {

std::string& tonedet_global_error() {
    thread_local std::string e;
    return e;
}

int tonedet_interval(int fs) { return fs < 8000 || fs > 48000 || fs % 10 != 0 ? 0 : fs / 10; }

int tonedet_gate(const fmd_tonedet_params* p, int fs, TonedetGate* out, std::string* err) {
    if (!p || !out) { *err = "null parameters"; return FMD_ERR_ARG; }
    const int M = tonedet_interval(fs);
    if (M == 0) { *err = "fs is not a multiple of 10 in 8000 ... 48000"; return FMD_ERR_ARG; }
    for (int k = 0; k < kTonedetSlots; k++) {
        const int f = p->freq_hz[k];
        if (f != 0 && (f < 1 || 2LL * f >= (long long)fs)) { *err = "freq_hz is neither 0 nor in 1 ... below fs / 2"; return FMD_ERR_ARG; }
        if (!(p->share_db[k] >= 0.0 && p->share_db[k] <= 60.0)) { *err = "share_db outside [0, 60]"; return FMD_ERR_ARG; }
        if (p->raise_intervals[k] < 1 || p->raise_intervals[k] > 36000 || p->clear_intervals[k] < 1 || p->clear_intervals[k] > 36000) {
            *err = "raise_intervals or clear_intervals outside 1 ... 36000";
            return FMD_ERR_ARG;
        }
    }
    if (!(p->floor_db < std::numeric_limits<double>::infinity())) { *err = "floor_db is neither finite nor -inf"; return FMD_ERR_ARG; }
    if (p->alarm_mask > 255u) { *err = "alarm_mask has a bit above bit 7"; return FMD_ERR_ARG; }
    out->min_e = p->floor_db == -std::numeric_limits<double>::infinity() ? 0.0 : std::pow(10.0, p->floor_db / 10.0) * (double)M;
    for (int k = 0; k < kTonedetSlots; k++) {
        out->c[k] = std::pow(10.0, -p->share_db[k] / 10.0);
        out->freq_hz[k] = p->freq_hz[k];
        out->raise_intervals[k] = p->raise_intervals[k];
        out->clear_intervals[k] = p->clear_intervals[k];
    }
    out->alarm_mask = p->alarm_mask;
    out->reserved = 0;
    return FMD_OK;
}

// libm's cos and libm's sin, each called on its own: an optimiser that sees both on one argument makes them one sincos(), whose results
// are not everywhere the bits of the two (18 of the 16000 values at fs = 8000 differ by an ulp)
__attribute__((noinline)) static double td_cos(double a) { return std::cos(a); }
__attribute__((noinline)) static double td_sin(double a) { return std::sin(a); }

void tonedet_table(int fs, double* tab) {
    for (int j = 0; j < fs; j++) {
        tab[2 * j] = td_cos(2.0 * M_PI * (double)j / (double)fs);
        tab[2 * j + 1] = td_sin(2.0 * M_PI * (double)j / (double)fs);
    }
}

}  // namespace fmd

static int td_readout_fail(int code, const char* msg) {
    fmd::tonedet_global_error() = msg;
    return code;
}

// pw of `slot` and mm over the newest `window` intervals, oldest first, and M
static int td_window(const fmd_tonedet_status* s, int fs, int slot, int window, const double* out, double* pw, double* mm, double* Md) {
    const int M = fmd::tonedet_interval(fs);
    if (!s || !out) return td_readout_fail(FMD_ERR_ARG, "null status or output");
    if (M == 0) return td_readout_fail(FMD_ERR_ARG, "fs is not a multiple of 10 in 8000 ... 48000");
    if (slot < 0 || slot >= fmd::kTonedetSlots) return td_readout_fail(FMD_ERR_ARG, "slot outside 0 ... 7");
    if (window < 1 || window > fmd::kTonedetRing) return td_readout_fail(FMD_ERR_ARG, "window outside 1 ... 30");
    if (s->intervals < (unsigned long long)window) return td_readout_fail(FMD_ERR_STATE, "fewer completed intervals than window");
    double a = 0.0, b = 0.0;
    for (unsigned long long g = s->intervals - (unsigned long long)window; g < s->intervals; g++) {
        a += s->ring_pw[slot][g % fmd::kTonedetRing];
        b += s->ring_mm[g % fmd::kTonedetRing];
    }
    *pw = a; *mm = b; *Md = (double)M;
    return FMD_OK;
}

extern "C" {

void fmd_tonedet_default_params(fmd_tonedet_params* p) {
    if (!p) return;
    static const int freq[fmd::kTonedetSlots] = {1000, 440, 400, 853, 960, 1050, 0, 0};
    static const double share[fmd::kTonedetSlots] = {3.0, 3.0, 3.0, 6.0, 6.0, 3.0, 3.0, 3.0};
    for (int k = 0; k < fmd::kTonedetSlots; k++) {
        p->freq_hz[k] = freq[k]; p->share_db[k] = share[k];
        p->raise_intervals[k] = 20; p->clear_intervals[k] = 5;
    }
    p->floor_db = -50.0;
    p->alarm_mask = 0u;
}

int fmd_tonedet_share_db(const fmd_tonedet_status* s, int fs, int slot, int window, double* db) {
    double pw, mm, M;
    const int rc = td_window(s, fs, slot, window, db, &pw, &mm, &M);
    if (rc != FMD_OK) return rc;
    *db = 10.0 * std::log10(2.0 * pw / (M * mm));
    return FMD_OK;
}

int fmd_tonedet_level_db(const fmd_tonedet_status* s, int fs, int slot, int window, double* db) {
    double pw, mm, M;
    const int rc = td_window(s, fs, slot, window, db, &pw, &mm, &M);
    if (rc != FMD_OK) return rc;
    *db = 10.0 * std::log10(2.0 * pw / (M * M * (double)window));
    return FMD_OK;
}

}  // extern "C"
