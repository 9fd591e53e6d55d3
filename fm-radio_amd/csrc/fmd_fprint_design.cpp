// Built with -ffp-contract=off -fno-fast-math (Makefile): every double operation is the one written, so the edges, the basis and the
// twiddles are the pure functions that tests/cpp/fprint_ref.c restates.
#include "fmd_fprint_design.h"

#include <cmath>
#include <cstdio>

namespace fmd {

std::string& fprint_global_error() {
    thread_local std::string e;
    return e;
}

int fprint_check(const fmd_fprint_config* c, std::string* err) {
    if (!c) { *err = "null configuration"; return FMD_ERR_ARG; }
    if (c->n_channels <= 0 || c->max_input_frames <= 0 || c->max_input_frames > (1LL << 30)) {
        *err = "n_channels is not positive or max_input_frames outside (0, 2^30]";
        return FMD_ERR_ARG;
    }
    if (c->fs < 8000 || c->fs > 48000) { *err = "fs outside 8000 ... 48000"; return FMD_ERR_ARG; }
    if (c->hop < 16 || c->hop > 1024 || c->hop % 16 != 0) { *err = "hop is not a multiple of 16 in 16 ... 1024"; return FMD_ERR_ARG; }
    if (c->n_sub != 4 && c->n_sub != 8 && c->n_sub != 16 && c->n_sub != 32) { *err = "n_sub is none of 4, 8, 16, 32"; return FMD_ERR_ARG; }
    if (c->n_bands < 2 || c->n_bands > kFprintMaxBands) { *err = "n_bands outside 2 ... 33"; return FMD_ERR_ARG; }
    if (!(c->f_min_hz > 0.0 && c->f_min_hz < c->f_max_hz && c->f_max_hz <= 1e9)) { *err = "not 0 < f_min_hz < f_max_hz"; return FMD_ERR_ARG; }
    return FMD_OK;
}

int fprint_layout(const fmd_fprint_config* c, FprintLayout* L, std::string* err) {
    const int H = c->hop, R = c->n_sub, B = c->n_bands, N = R * H;
    FprintLayout l{};
    l.N = N;
    for (int b = 0; b <= B; b++) {
        const double f = c->f_min_hz * std::pow(c->f_max_hz / c->f_min_hz, (double)b / (double)B);
        const double k = std::floor(f * (double)N / (double)c->fs + 0.5);
        if (!(k <= (double)(N / 2 - 1))) { *err = "a band edge lies above bin N / 2 - 1"; return FMD_ERR_ARG; }
        l.edges[b] = (int)k;
    }
    if (l.edges[0] < 1) { *err = "the lowest band edge lies below bin 1"; return FMD_ERR_ARG; }
    for (int b = 0; b < B; b++)
        if (l.edges[b] >= l.edges[b + 1]) {
            char buf[96];
            snprintf(buf, sizeof(buf), "band %d is empty (bins %d ... %d)", b, l.edges[b], l.edges[b + 1]);
            *err = buf;
            return FMD_ERR_ARG;
        }
    l.first_bin = l.edges[0] - 1;
    l.K = l.edges[B] - l.edges[0] + 2;
    l.Kp = (l.K + kFprintTile - 1) / kFprintTile * kFprintTile;
    long long piece = kFprintScratchBytes / (8LL * l.Kp);
    if (piece < 2) piece = 2;
    if (piece > kFprintMaxPiece) piece = kFprintMaxPiece;
    const long long most = (c->max_input_frames + H - 1) / H;
    if (piece > most) piece = most;
    l.piece = (int)piece;
    l.piece_frames = piece * H;
    const int span = kFprintChunk + 2;
    l.lds_floats = (R - 1 + l.piece) * span * 2 + l.piece * span * 2 + l.piece * kFprintChunk + (l.piece + 1) * kFprintMaxBands + 2 * 32 + (kFprintMaxBands + 1);
    *L = l;
    return FMD_OK;
}

long long fprint_bytes(const fmd_fprint_config* c, const FprintLayout& L, long long C) {
    const long long row = 2LL * L.Kp * 4;
    return C * (32 + 4LL * c->hop + 4LL * kFprintMaxBands + (c->n_sub - 1) * row + L.piece * row + 4 + 4) + 4 + (long long)c->hop * row + 2 * 32 * 4 +
           (kFprintMaxBands + 1) * 4;
}

// libm's cos and libm's sin, each called on its own (an optimiser that sees both on one argument makes them one sincos())
__attribute__((noinline)) static double fp_cos(double a) { return std::cos(a); }
__attribute__((noinline)) static double fp_sin(double a) { return std::sin(a); }

}  // namespace fmd

static int fp_fail(int code, const std::string& msg) {
    fmd::fprint_global_error() = msg;
    return code;
}

extern "C" {

int fmd_fprint_default_config(int fs, fmd_fprint_config* cfg) {
    if (!cfg) return fp_fail(FMD_ERR_ARG, "null configuration");
    if (fs < 8000 || fs > 48000) return fp_fail(FMD_ERR_ARG, "fs outside 8000 ... 48000");
    cfg->n_channels = 1;
    cfg->fs = fs;
    cfg->hop = 16 * ((fs * 23 + 16000) / 32000);     // fs * 0.0115 / 16, rounded
    cfg->n_sub = 32;
    cfg->n_bands = 33;
    cfg->f_min_hz = 300.0;
    cfg->f_max_hz = 2000.0;
    cfg->max_input_frames = 65536;
    cfg->device = -1;
    return FMD_OK;
}

int fmd_fprint_bins(const fmd_fprint_config* cfg) {
    std::string err;
    fmd::FprintLayout L;
    if (fmd::fprint_check(cfg, &err) != FMD_OK || fmd::fprint_layout(cfg, &L, &err) != FMD_OK) return fp_fail(FMD_ERR_ARG, err);
    return L.K;
}

int fmd_fprint_design(const fmd_fprint_config* cfg, float* bc, float* bs, float* wc, float* ws, int* edges, fmd_fprint_design_t* out) {
    std::string err;
    fmd::FprintLayout L;
    if (fmd::fprint_check(cfg, &err) != FMD_OK || fmd::fprint_layout(cfg, &L, &err) != FMD_OK) return fp_fail(FMD_ERR_ARG, err);
    const int H = cfg->hop, R = cfg->n_sub, N = L.N, K = L.K;
    if (bc || bs)
        for (int n = 0; n < H; n++)
            for (int k = 0; k < K; k++) {
                const long long idx = ((long long)(L.first_bin + k) * (long long)n) % (long long)N;
                const double phi = 2.0 * M_PI * (double)idx / (double)N;
                if (bc) bc[(size_t)n * (size_t)K + (size_t)k] = (float)fmd::fp_cos(phi);
                if (bs) bs[(size_t)n * (size_t)K + (size_t)k] = (float)(-fmd::fp_sin(phi));
            }
    for (int q = 0; q < R; q++) {
        const double a = 2.0 * M_PI * (double)q / (double)R;
        float c = (float)fmd::fp_cos(a), s = (float)fmd::fp_sin(a);
        if (q % (R / 4) == 0) {                        // the quarter turns are exact
            static const float qc[4] = {1.0f, 0.0f, -1.0f, 0.0f}, qs[4] = {0.0f, 1.0f, 0.0f, -1.0f};
            c = qc[q / (R / 4)]; s = qs[q / (R / 4)];
        }
        if (wc) wc[q] = c;
        if (ws) ws[q] = s;
    }
    if (edges)
        for (int b = 0; b <= cfg->n_bands; b++) edges[b] = L.edges[b];
    if (out) { out->n_bins = K; out->first_bin = L.first_bin; }
    return FMD_OK;
}

long long fmd_fprint_max_prints(int hop, long long n) {
    if (hop < 16 || hop > 1024 || n < 0 || n > (1LL << 40)) return fp_fail(FMD_ERR_ARG, "hop outside 16 ... 1024 or n outside [0, 2^40]");
    return (n + (long long)hop - 1) / (long long)hop;
}

long long fmd_fprint_state_bytes(const fmd_fprint_config* cfg, int channels) {
    std::string err;
    fmd::FprintLayout L;
    if (channels <= 0) return fp_fail(FMD_ERR_ARG, "channels is not positive");
    if (fmd::fprint_check(cfg, &err) != FMD_OK || fmd::fprint_layout(cfg, &L, &err) != FMD_OK) return fp_fail(FMD_ERR_ARG, err);
    return fmd::fprint_bytes(cfg, L, channels);
}

}  // extern "C"
