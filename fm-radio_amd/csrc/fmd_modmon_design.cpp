// Built with -ffp-contract=off -fno-fast-math (Makefile): every double operation is the one written, so the design and the read-out are
// the pure functions that tests/cpp/modmon_ref.c restates.
#include "fmd_modmon_design.h"

#include <cmath>
#include <cstring>
#include <limits>

#include "fmd_bessel.h"

namespace fmd {

std::string& modmon_global_error() {
    thread_local std::string e;
    return e;
}

static double modmon_sinc(double x) {
    const double pi = 3.14159265358979323846;
    return x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
}

int modmon_design(int fs, fmd_modmon_design_t* out, std::string* err) {
    if (!out) { *err = "null design"; return FMD_ERR_ARG; }
    if (fs < 192000 || fs > 384000 || fs % 1000 != 0) { *err = "fs " + std::to_string(fs) + " is not a multiple of 1000 in 192000 ... 384000"; return FMD_ERR_ARG; }
    const double pi = 3.14159265358979323846;
    std::memset(out, 0, sizeof(*out));
    int a = fs, b = 19000;
    while (b) { const int t = a % b; a = b; b = t; }
    out->fs = fs;
    out->M = fs / 20;
    out->P = fs / a;
    out->hz_per_rad = (double)fs / (2.0 * pi);
    {   // MPX low-pass: a Kaiser-windowed sinc
        const double w = 2.0 * 76000.0 / (double)fs, i0b = bessel_i0(5.0);
        double g[kModmonTaps], sum = 0.0;
        for (int i = 0; i < kModmonTaps; i++) {
            const double x = w * (double)(i - 16), r = (double)(i - 16) / 16.0;
            g[i] = ((w * modmon_sinc(x)) * bessel_i0(5.0 * std::sqrt(1.0 - r * r))) / i0b;
            sum += g[i];
        }
        for (int i = 0; i < kModmonTaps; i++) out->h[i] = (float)(g[i] / sum);
    }
    for (int k = 0; k < out->P; k++) {
        const long long m = (19000LL * k) % fs;
        const double ang = (2.0 * pi * (double)m) / (double)fs;
        out->pilot_cos[k] = std::cos(ang);
        out->pilot_sin[k] = std::sin(ang);
    }
    {
        double re = 0.0, im = 0.0;
        for (int i = 0; i < kModmonTaps; i++) {
            const double ang = (2.0 * pi * (double)(19000 * i)) / (double)fs;
            re += (double)out->h[i] * std::cos(ang);
            im += (double)out->h[i] * std::sin(ang);
        }
        out->pilot_gain = std::sqrt(re * re + im * im) * modmon_sinc(19000.0 / (double)fs);
    }
    for (int j = 0; j <= kModmonBins; j++) out->edge[j] = kModmonBinHz * (double)j;
    return FMD_OK;
}

}  // namespace fmd

static int mm_readout_fail(int code, const char* msg) {
    fmd::modmon_global_error() = msg;
    return code;
}

extern "C" {

int fmd_modmon_design(int fs, fmd_modmon_design_t* out) { return fmd::modmon_design(fs, out, &fmd::modmon_global_error()); }

int fmd_modmon_deviation_hz(const fmd_modmon_status* s, const fmd_modmon_design_t* d, double* hz) {
    if (!s || !d || !hz) return mm_readout_fail(FMD_ERR_ARG, "null status, design or output");
    if (s->intervals == 0) return mm_readout_fail(FMD_ERR_STATE, "no interval is complete yet");
    *hz = 0.5 * ((double)s->last_hi - (double)s->last_lo) * d->hz_per_rad;
    return FMD_OK;
}

int fmd_modmon_offset_hz(const fmd_modmon_status* s, const fmd_modmon_design_t* d, double* hz) {
    if (!s || !d || !hz) return mm_readout_fail(FMD_ERR_ARG, "null status, design or output");
    if (s->intervals == 0) return mm_readout_fail(FMD_ERR_STATE, "no interval is complete yet");
    *hz = s->last_s1 / (double)d->M;
    return FMD_OK;
}

int fmd_modmon_pilot_hz(const fmd_modmon_status* s, const fmd_modmon_design_t* d, double* hz) {
    if (!s || !d || !hz) return mm_readout_fail(FMD_ERR_ARG, "null status, design or output");
    if (s->intervals == 0) return mm_readout_fail(FMD_ERR_STATE, "no interval is complete yet");
    *hz = 2.0 * std::sqrt(std::fma(s->last_sc, s->last_sc, s->last_ss * s->last_ss)) / (double)d->M / d->pilot_gain;
    return FMD_OK;
}

int fmd_modmon_mpx_power_dbr(const fmd_modmon_status* s, const fmd_modmon_design_t* d, int window_s, double* dbr) {
    if (!s || !d || !dbr) return mm_readout_fail(FMD_ERR_ARG, "null status, design or output");
    if (window_s < 1 || window_s > fmd::kModmonRing) return mm_readout_fail(FMD_ERR_ARG, "window_s outside 1 ... 60");
    if (s->seconds < (unsigned long long)window_s) return mm_readout_fail(FMD_ERR_STATE, "fewer completed seconds than window_s");
    double e = 0.0, f = 0.0;
    unsigned long long k = 0;
    for (unsigned long long t = s->seconds - (unsigned long long)window_s; t < s->seconds; t++) {
        e += s->sec_e[t % fmd::kModmonRing];
        f += s->sec_f[t % fmd::kModmonRing];
        k += s->sec_n[t % fmd::kModmonRing];
    }
    if (k == 0) return mm_readout_fail(FMD_ERR_STATE, "no interval of the window was classified");
    const double N = (double)d->M * (double)k;
    const double v = e / N - (f / N) * (f / N);
    *dbr = v <= 0.0 ? -std::numeric_limits<double>::infinity() : 10.0 * std::log10(2.0 * v / (19000.0 * 19000.0));
    return FMD_OK;
}

int fmd_modmon_exceedance(const unsigned* hist, unsigned over, int limit_hz, double* fraction, unsigned long long* count) {
    if (!hist || !fraction || !count) return mm_readout_fail(FMD_ERR_ARG, "null histogram or output");
    if (limit_hz < 0 || limit_hz > 150000 || limit_hz % 500 != 0) return mm_readout_fail(FMD_ERR_ARG, "limit_hz is not a multiple of 500 in 0 ... 150000");
    unsigned long long n = over, c = over;
    for (int j = 0; j < fmd::kModmonBins; j++) {
        n += hist[j];
        if (j >= limit_hz / 500) c += hist[j];
    }
    if (n == 0) return mm_readout_fail(FMD_ERR_STATE, "the histogram is empty");
    *count = c;
    *fraction = (double)c / (double)n;
    return FMD_OK;
}

int fmd_modmon_percentile(const unsigned* hist, unsigned over, double q, double* hz) {
    if (!hist || !hz) return mm_readout_fail(FMD_ERR_ARG, "null histogram or output");
    if (!(q >= 0.0 && q <= 1.0)) return mm_readout_fail(FMD_ERR_ARG, "q outside 0 ... 1");
    unsigned long long n = over;
    for (int j = 0; j < fmd::kModmonBins; j++) n += hist[j];
    if (n == 0) return mm_readout_fail(FMD_ERR_STATE, "the histogram is empty");
    const unsigned long long rank = (unsigned long long)std::floor(q * (double)(n - 1) + 0.5);
    unsigned long long cum = 0;
    for (int j = 0; j < fmd::kModmonBins; j++) {
        cum += hist[j];
        if (cum > rank) { *hz = fmd::kModmonBinHz * (double)j + 250.0; return FMD_OK; }
    }
    *hz = 150000.0;
    return FMD_OK;
}

}  // extern "C"
