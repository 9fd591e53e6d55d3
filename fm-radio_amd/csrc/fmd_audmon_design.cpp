// Built with -ffp-contract=off -fno-fast-math (Makefile): every double operation is the one written, so the thresholds and the read-outs
// are the pure functions that tests/cpp/audmon_ref.c restates.
#include "fmd_audmon_design.h"

#include <cmath>
#include <limits>

namespace fmd {

std::string& audmon_global_error() {
    thread_local std::string e;
    return e;
}

int audmon_interval(int fs) { return fs < 8000 || fs > 192000 || fs % 10 != 0 ? 0 : fs / 10; }

int audmon_gate(const fmd_audmon_params* p, int M, AudmonGate* out, std::string* err) {
    if (!p || !out) { *err = "null parameters"; return FMD_ERR_ARG; }
    if (!(p->silence_db < std::numeric_limits<double>::infinity())) { *err = "silence_db is neither finite nor -inf"; return FMD_ERR_ARG; }
    if (!(p->loss_db > 0.0 && p->loss_db <= 120.0)) { *err = "loss_db outside (0, 120]"; return FMD_ERR_ARG; }
    if (!(p->antiphase_corr > 0.0 && p->antiphase_corr < 1.0)) { *err = "antiphase_corr outside (0, 1)"; return FMD_ERR_ARG; }
    if (!(p->mono_db > 0.0 && p->mono_db <= 120.0)) { *err = "mono_db outside (0, 120]"; return FMD_ERR_ARG; }
    for (int k = 0; k < kAudmonDetectors; k++)
        if (p->raise_intervals[k] < 1 || p->raise_intervals[k] > 36000 || p->clear_intervals[k] < 1 || p->clear_intervals[k] > 36000) {
            *err = "raise_intervals or clear_intervals outside 1 ... 36000";
            return FMD_ERR_ARG;
        }
    if (p->alarm_mask > 31u) { *err = "alarm_mask has a bit above bit 4"; return FMD_ERR_ARG; }
    out->min_e = p->silence_db == -std::numeric_limits<double>::infinity() ? 0.0 : std::pow(10.0, p->silence_db / 10.0) * (2.0 * (double)M);
    out->c_loss = std::pow(10.0, -p->loss_db / 10.0);
    out->c_anti = p->antiphase_corr * p->antiphase_corr;
    out->c_mono = std::pow(10.0, -p->mono_db / 10.0);
    for (int k = 0; k < kAudmonDetectors; k++) { out->raise_intervals[k] = p->raise_intervals[k]; out->clear_intervals[k] = p->clear_intervals[k]; }
    out->alarm_mask = p->alarm_mask;
    out->reserved = 0;
    return FMD_OK;
}

}  // namespace fmd

static int am_readout_fail(int code, const char* msg) {
    fmd::audmon_global_error() = msg;
    return code;
}

// ll, rr, lr over the newest `window` intervals, oldest first, and N
static int am_window(const fmd_audmon_status* s, int fs, int window, const double* out, double* ll, double* rr, double* lr, double* N) {
    const int M = fmd::audmon_interval(fs);
    if (!s || !out) return am_readout_fail(FMD_ERR_ARG, "null status or output");
    if (M == 0) return am_readout_fail(FMD_ERR_ARG, "fs is not a multiple of 10 in 8000 ... 192000");
    if (window < 1 || window > fmd::kAudmonRing) return am_readout_fail(FMD_ERR_ARG, "window outside 1 ... 30");
    if (s->intervals < (unsigned long long)window) return am_readout_fail(FMD_ERR_STATE, "fewer completed intervals than window");
    double a = 0.0, b = 0.0, c = 0.0;
    for (unsigned long long g = s->intervals - (unsigned long long)window; g < s->intervals; g++) {
        a += s->ring_ll[g % fmd::kAudmonRing];
        b += s->ring_rr[g % fmd::kAudmonRing];
        c += s->ring_lr[g % fmd::kAudmonRing];
    }
    *ll = a; *rr = b; *lr = c;
    *N = (double)M * (double)window;
    return FMD_OK;
}

extern "C" {

void fmd_audmon_default_params(fmd_audmon_params* p) {
    if (!p) return;
    static const int raise[fmd::kAudmonDetectors] = {100, 100, 100, 50, 100};
    p->silence_db = -60.0;
    p->loss_db = 30.0;
    p->antiphase_corr = 0.5;
    p->mono_db = 40.0;
    for (int k = 0; k < fmd::kAudmonDetectors; k++) { p->raise_intervals[k] = raise[k]; p->clear_intervals[k] = 10; }
    p->alarm_mask = FMD_AUDMON_SILENCE | FMD_AUDMON_LEFT_LOST | FMD_AUDMON_RIGHT_LOST | FMD_AUDMON_ANTIPHASE;
}

int fmd_audmon_level_db(const fmd_audmon_status* s, int fs, int rail, int window, double* db) {
    double ll, rr, lr, N;
    if (rail < 0 || rail > 2) return am_readout_fail(FMD_ERR_ARG, "rail is not 0 (L), 1 (R) or 2 (both)");
    const int rc = am_window(s, fs, window, db, &ll, &rr, &lr, &N);
    if (rc != FMD_OK) return rc;
    *db = rail == 0 ? 10.0 * std::log10(ll / N) : rail == 1 ? 10.0 * std::log10(rr / N) : 10.0 * std::log10((ll + rr) / (2.0 * N));
    return FMD_OK;
}

int fmd_audmon_balance_db(const fmd_audmon_status* s, int fs, int window, double* db) {
    double ll, rr, lr, N;
    const int rc = am_window(s, fs, window, db, &ll, &rr, &lr, &N);
    if (rc != FMD_OK) return rc;
    *db = 10.0 * std::log10(ll / rr);
    return FMD_OK;
}

int fmd_audmon_correlation(const fmd_audmon_status* s, int fs, int window, double* corr) {
    double ll, rr, lr, N;
    const int rc = am_window(s, fs, window, corr, &ll, &rr, &lr, &N);
    if (rc != FMD_OK) return rc;
    *corr = lr / std::sqrt(ll * rr);
    return FMD_OK;
}

int fmd_audmon_side_mid_db(const fmd_audmon_status* s, int fs, int window, double* db) {
    double ll, rr, lr, N;
    const int rc = am_window(s, fs, window, db, &ll, &rr, &lr, &N);
    if (rc != FMD_OK) return rc;
    *db = 10.0 * std::log10(std::fma(-2.0, lr, ll + rr) / std::fma(2.0, lr, ll + rr));
    return FMD_OK;
}

}  // extern "C"
