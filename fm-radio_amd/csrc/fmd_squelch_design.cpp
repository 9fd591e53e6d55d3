// Built with -ffp-contract=off -fno-fast-math (Makefile): every double operation is the one written, so the thresholds and the read-out
// are the pure functions that tests/cpp/squelch_ref.c restates.
#include "fmd_squelch_design.h"

#include <cmath>
#include <limits>

namespace fmd {

std::string& squelch_global_error() {
    thread_local std::string e;
    return e;
}

int squelch_interval(int fs) { return fs < 192000 || fs > 384000 || fs % 1000 != 0 ? 0 : fs / 20; }

int squelch_gate(const fmd_squelch_params* p, int M, SquelchGate* out, std::string* err) {
    if (!p || !out) { *err = "null parameters"; return FMD_ERR_ARG; }
    if (!(p->close_db >= 0.0 && p->close_db <= p->open_db && p->open_db <= 60.0)) { *err = "thresholds outside 0 <= close_db <= open_db <= 60"; return FMD_ERR_ARG; }
    if (!(p->min_level_db < std::numeric_limits<double>::infinity())) { *err = "min_level_db is neither finite nor -inf"; return FMD_ERR_ARG; }
    if (p->open_intervals < 1 || p->open_intervals > 1000 || p->close_intervals < 1 || p->close_intervals > 1000) {
        *err = "open_intervals or close_intervals outside 1 ... 1000";
        return FMD_ERR_ARG;
    }
    if (p->mode != FMD_SQUELCH_AUTO && p->mode != FMD_SQUELCH_FORCE_OPEN && p->mode != FMD_SQUELCH_FORCE_CLOSED) { *err = "mode is not one of FMD_SQUELCH_*"; return FMD_ERR_ARG; }
    out->c_open = fmd_squelch_threshold(p->open_db);
    out->c_close = fmd_squelch_threshold(p->close_db);
    out->min_s2 = p->min_level_db == -std::numeric_limits<double>::infinity() ? 0.0 : std::pow(10.0, p->min_level_db / 10.0) * (double)M;
    out->open_intervals = p->open_intervals;
    out->close_intervals = p->close_intervals;
    out->mode = p->mode;
    out->reserved = 0;
    return FMD_OK;
}

}  // namespace fmd

static int sq_readout_fail(int code, const char* msg) {
    fmd::squelch_global_error() = msg;
    return code;
}

// e2, e4 over the newest `window` intervals, oldest first, and N
static int sq_window(const fmd_squelch_status* s, int fs, int window, double* e2, double* e4, double* N) {
    const int M = fmd::squelch_interval(fs);
    if (!s) return sq_readout_fail(FMD_ERR_ARG, "null status or output");
    if (M == 0) return sq_readout_fail(FMD_ERR_ARG, "fs is not a multiple of 1000 in 192000 ... 384000");
    if (window < 1 || window > fmd::kSquelchRing) return sq_readout_fail(FMD_ERR_ARG, "window outside 1 ... 20");
    if (s->intervals < (unsigned long long)window) return sq_readout_fail(FMD_ERR_STATE, "fewer completed intervals than window");
    double a = 0.0, b = 0.0;
    for (unsigned long long g = s->intervals - (unsigned long long)window; g < s->intervals; g++) {
        a += s->ring_s2[g % fmd::kSquelchRing];
        b += s->ring_s4[g % fmd::kSquelchRing];
    }
    *e2 = a; *e4 = b;
    *N = (double)M * (double)window;
    return FMD_OK;
}

extern "C" {

void fmd_squelch_default_params(fmd_squelch_params* p) {
    if (!p) return;
    p->open_db = 10.0;
    p->close_db = 7.0;
    p->min_level_db = -std::numeric_limits<double>::infinity();
    p->open_intervals = 2;
    p->close_intervals = 10;
    p->mode = FMD_SQUELCH_AUTO;
}

double fmd_squelch_threshold(double db) {
    const double k = std::pow(10.0, db / 10.0);
    return (k * k) / ((1.0 + k) * (1.0 + k));
}

int fmd_squelch_level_db(const fmd_squelch_status* s, int fs, double* db) {
    double e2, e4, N;
    if (!db) return sq_readout_fail(FMD_ERR_ARG, "null status or output");
    const int rc = sq_window(s, fs, 1, &e2, &e4, &N);
    if (rc != FMD_OK) return rc;
    *db = 10.0 * std::log10(s->ring_s2[(s->intervals - 1) % fmd::kSquelchRing] / N);
    return FMD_OK;
}

int fmd_squelch_powers(const fmd_squelch_status* s, int fs, int window, double* carrier, double* noise) {
    double e2, e4, N;
    if (!carrier || !noise) return sq_readout_fail(FMD_ERR_ARG, "null status or output");
    const int rc = sq_window(s, fs, window, &e2, &e4, &N);
    if (rc != FMD_OK) return rc;
    const double d = std::fma(-N, e4, 2.0 * e2 * e2);
    if (d <= 0.0) { *carrier = 0.0; *noise = e2 / N; return FMD_OK; }
    const double c = std::sqrt(d) / N;
    *carrier = c;
    *noise = e2 / N - c;
    return FMD_OK;
}

int fmd_squelch_cnr_db(const fmd_squelch_status* s, int fs, int window, double* db) {
    double e2, e4, N;
    if (!db) return sq_readout_fail(FMD_ERR_ARG, "null status or output");
    const int rc = sq_window(s, fs, window, &e2, &e4, &N);
    if (rc != FMD_OK) return rc;
    const double d = std::fma(-N, e4, 2.0 * e2 * e2);
    if (d <= 0.0) { *db = -std::numeric_limits<double>::infinity(); return FMD_OK; }
    const double c = std::sqrt(d) / N;
    const double nz = e2 / N - c;
    *db = nz <= 0.0 ? std::numeric_limits<double>::infinity() : 10.0 * std::log10(c / nz);
    return FMD_OK;
}

}  // extern "C"
