// Built with -ffp-contract=off -fno-fast-math (Makefile): every double operation is the one written, so the window, the table and the
// filterbank are the pure functions that tests/cpp/logmel_ref.c restates.
#include "fmd_logmel_design.h"

#include <cfloat>
#include <cmath>
#include <vector>

#include "fmd_logmel_math.h"

namespace fmd {

std::string& logmel_global_error() {
    thread_local std::string e;
    return e;
}

int logmel_check(const fmd_logmel_config* c, std::string* err) {
    if (!c) { *err = "null configuration"; return FMD_ERR_ARG; }
    if (c->n_channels <= 0 || c->max_input_frames <= 0 || c->max_input_frames > (1LL << 30)) {
        *err = "n_channels is not positive or max_input_frames outside (0, 2^30]";
        return FMD_ERR_ARG;
    }
    if (c->fs < 8000 || c->fs > 48000) { *err = "fs outside 8000 ... 48000"; return FMD_ERR_ARG; }
    if (c->win < 64 || c->win > 2048 || c->win % 16 != 0) { *err = "win is not a multiple of 16 in 64 ... 2048"; return FMD_ERR_ARG; }
    if (c->hop < 16 || c->hop > c->win) { *err = "hop outside 16 ... win"; return FMD_ERR_ARG; }
    if (c->n_mels < 1 || c->n_mels > 128) { *err = "n_mels outside 1 ... 128"; return FMD_ERR_ARG; }
    if (!(c->f_min_hz >= 0.0 && c->f_min_hz < c->f_max_hz && c->f_max_hz <= 0.5 * (double)c->fs)) {
        *err = "not 0 <= f_min_hz < f_max_hz <= fs / 2";
        return FMD_ERR_ARG;
    }
    if (c->mel_scale != 0 && c->mel_scale != 1) { *err = "mel_scale is neither 0 (Slaney) nor 1 (HTK)"; return FMD_ERR_ARG; }
    if (c->out_mode != 0 && c->out_mode != 1) { *err = "out_mode is neither 0 (mel power) nor 1 (log10)"; return FMD_ERR_ARG; }
    if (!(c->log_floor >= FLT_MIN && c->log_floor <= FLT_MAX)) { *err = "log_floor is not finite or below FLT_MIN"; return FMD_ERR_ARG; }
    return FMD_OK;
}

int logmel_bins(const fmd_logmel_config* c) {
    const int half = c->win / 2;
    const double top = std::floor(c->f_max_hz * (double)c->win / (double)c->fs);
    return (top < (double)half ? (int)top : half) + 1;
}

LogmelLayout logmel_layout(const fmd_logmel_config* c) {
    LogmelLayout L{};
    const int N = c->win;
    L.K = logmel_bins(c);
    L.Kp = (L.K + kLogmelTile - 1) / kLogmelTile * kLogmelTile;
    L.Mp = (c->n_mels + kLogmelTile - 1) / kLogmelTile * kLogmelTile;
    const int budget = kLogmelLdsBytes / 4, fixed = 3 * N + kLogmelTile;
    int rows = kLogmelTile;
    while (rows > 1 && fixed + (rows - 1) * c->hop + N + rows * L.Kp > budget) rows--;   // (one row always fits: 3 N + 16 + N + Kp <= 9248)
    L.rows = rows;
    L.span = (rows - 1) * c->hop + N;
    L.off_w = 0;
    L.off_tab = N;
    L.off_m = 3 * N;
    L.off_p = L.off_m + L.span;
    L.off_nf = L.off_p + rows * L.Kp;
    L.total = L.off_nf + kLogmelTile;
    return L;
}

// libm's cos and libm's sin, each called on its own: an optimiser that sees both on one argument makes them one sincos(), whose results
// are not everywhere the bits of the two
__attribute__((noinline)) static double lm_cos(double a) { return std::cos(a); }
__attribute__((noinline)) static double lm_sin(double a) { return std::sin(a); }

static double lm_mel(double f, int scale) {
    if (scale == 1) return 2595.0 * std::log10(1.0 + f / 700.0);
    return f < 1000.0 ? f / (200.0 / 3.0) : 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0);
}
static double lm_mel_inv(double m, int scale) {
    if (scale == 1) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    return m < 15.0 ? m * (200.0 / 3.0) : 1000.0 * std::exp((m - 15.0) * (std::log(6.4) / 27.0));
}

}  // namespace fmd

static int lm_fail(int code, const std::string& msg) {
    fmd::logmel_global_error() = msg;
    return code;
}

extern "C" {

int fmd_logmel_default_config(int fs, fmd_logmel_config* cfg) {
    if (!cfg) return lm_fail(FMD_ERR_ARG, "null configuration");
    if (fs < 8000 || fs > 48000) return lm_fail(FMD_ERR_ARG, "fs outside 8000 ... 48000");
    cfg->n_channels = 1;
    cfg->fs = fs;
    cfg->win = (fs / 40 + 15) / 16 * 16;
    cfg->hop = fs / 100;
    cfg->n_mels = 80;
    cfg->f_min_hz = 0.0;
    cfg->f_max_hz = 0.5 * (double)fs < 8000.0 ? 0.5 * (double)fs : 8000.0;
    cfg->mel_scale = 0;
    cfg->out_mode = 1;
    cfg->log_floor = 1e-10f;
    cfg->max_input_frames = 65536;
    cfg->device = -1;
    return FMD_OK;
}

int fmd_logmel_bins(const fmd_logmel_config* cfg) {
    std::string err;
    if (fmd::logmel_check(cfg, &err) != FMD_OK) return lm_fail(FMD_ERR_ARG, err);
    return fmd::logmel_bins(cfg);
}

int fmd_logmel_design(const fmd_logmel_config* cfg, float* w, float* tc, float* ts, float* fb, fmd_logmel_design_t* out) {
    std::string err;
    if (fmd::logmel_check(cfg, &err) != FMD_OK) return lm_fail(FMD_ERR_ARG, err);
    const int N = cfg->win, K = fmd::logmel_bins(cfg), nm = cfg->n_mels, scale = cfg->mel_scale;
    for (int n = 0; n < N; n++) {
        const double a = 2.0 * M_PI * (double)n / (double)N;
        if (w) w[n] = (float)(0.5 - 0.5 * fmd::lm_cos(a));
        if (tc) tc[n] = (float)fmd::lm_cos(a);
        if (ts) ts[n] = (float)fmd::lm_sin(a);
    }
    std::vector<double> F((size_t)nm + 2);
    const double m0 = fmd::lm_mel(cfg->f_min_hz, scale), m1 = fmd::lm_mel(cfg->f_max_hz, scale);
    for (int i = 0; i < nm + 2; i++) F[(size_t)i] = fmd::lm_mel_inv(m0 + (double)i * (m1 - m0) / (double)(nm + 1), scale);
    int empty = 0;
    for (int j = 0; j < nm; j++) {
        const double Fa = F[(size_t)j], Fb = F[(size_t)j + 1], Fc = F[(size_t)j + 2];
        const double s = scale == 0 ? 2.0 / (Fc - Fa) : 1.0;
        bool any = false;
        for (int k = 0; k < K; k++) {
            const double fk = (double)k * (double)cfg->fs / (double)N;
            const double up = (fk - Fa) / (Fb - Fa), down = (Fc - fk) / (Fc - Fb);
            const double t = up < down ? up : down;
            const float v = (float)((t > 0.0 ? t : 0.0) * s);
            if (fb) fb[(size_t)j * (size_t)K + (size_t)k] = v;
            any = any || v != 0.0f;
        }
        if (!any) empty++;
    }
    if (out) { out->n_bins = K; out->empty_bands = empty; }
    return FMD_OK;
}

long long fmd_logmel_max_frames(int hop, long long n) {
    if (hop < 16 || hop > 2048 || n < 0 || n > (1LL << 40)) return lm_fail(FMD_ERR_ARG, "hop outside 16 ... 2048 or n outside [0, 2^40]");
    return (n + (long long)hop - 1) / (long long)hop;
}

float fmd_logmel_flog10(float x) { return fmd::flog10(x); }

}  // extern "C"
