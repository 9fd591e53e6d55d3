// Built with -ffp-contract=off -fno-fast-math (Makefile): every double operation is the one written, so the design and the read-out are
// the pure functions that tests/cpp/meter_ref.c restates.
#include "fmd_meter_design.h"

#include <cmath>
#include <limits>

#include "fmd_bessel.h"

namespace fmd {

std::string& meter_global_error() {
    thread_local std::string e;
    return e;
}

int meter_design(int fs, fmd_meter_design_t* out, std::string* err) {
    if (!out) { *err = "null design"; return FMD_ERR_ARG; }
    if (fs < 8000 || fs > 192000 || fs % 10 != 0) { *err = "fs " + std::to_string(fs) + " is not a multiple of 10 in 8000 ... 192000"; return FMD_ERR_ARG; }
    const double pi = 3.14159265358979323846;
    {   // pre-filter: high shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / (double)fs);
        volatile double ten = 10.0;            // (read at run time: the host libm's pow, not a compiler's folded constant)
        const double Vh = std::pow(ten, G / 20.0);
        const double Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        out->pre_b[0] = (Vh + Vb * K / Q + K * K) / a0;
        out->pre_b[1] = 2.0 * (K * K - Vh) / a0;
        out->pre_b[2] = (Vh - Vb * K / Q + K * K) / a0;
        out->pre_a[0] = 1.0;
        out->pre_a[1] = 2.0 * (K * K - 1.0) / a0;
        out->pre_a[2] = (1.0 - K / Q + K * K) / a0;
    }
    {   // RLB high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / (double)fs);
        const double a0 = 1.0 + K / Q + K * K;
        out->rlb_b[0] = 1.0;
        out->rlb_b[1] = -2.0;
        out->rlb_b[2] = 1.0;
        out->rlb_a[0] = 1.0;
        out->rlb_a[1] = 2.0 * (K * K - 1.0) / a0;
        out->rlb_a[2] = (1.0 - K / Q + K * K) / a0;
    }
    out->frames_per_subblock = fs / 10;
    for (int j = 0; j <= kMeterBins; j++) out->edge[j] = std::pow(10.0, ((-70.0 + 0.1 * (double)j) + 0.691) / 10.0);
    for (int j = 0; j < kMeterBins; j++) out->centre[j] = std::pow(10.0, (((-70.0 + 0.1 * (double)j) + 0.05) + 0.691) / 10.0);
    return FMD_OK;
}

// The true-peak interpolator (include/fmdemod.h, "tp design"): a Kaiser-windowed sinc at L fs, cut into its L phases.
int meter_tp_design(int fs, fmd_meter_tp_design_t* out, std::string* err) {
    if (!out) { *err = "null design"; return FMD_ERR_ARG; }
    if (fs < 8000 || fs > 192000 || fs % 10 != 0) { *err = "fs " + std::to_string(fs) + " is not a multiple of 10 in 8000 ... 192000"; return FMD_ERR_ARG; }
    const double pi = 3.14159265358979323846, beta = 5.0;
    const int L = fs < 88200 ? 4 : fs < 176400 ? 2 : 1, T = kMeterTpTaps, N = L * T;
    const double c = (double)(N / 2), i0b = bessel_i0(beta);
    out->L = L;
    out->taps_per_phase = T;
    for (int p = 0; p < 3; p++)
        for (int k = 0; k < T; k++) out->taps[p][k] = 0.0f;
    for (int p = 1; p < L; p++) {
        double g[kMeterTpTaps], sum = 0.0;
        for (int k = 0; k < T; k++) {
            const double t = (double)(k * L + p) - c, x = t / (double)L, r = t / c;
            const double s = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
            g[k] = s * bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b;
            sum += g[k];
        }
        for (int k = 0; k < T; k++) out->taps[p - 1][k] = (float)(g[k] / sum);
    }
    return FMD_OK;
}

}  // namespace fmd

extern "C" {

int fmd_meter_design(int fs, fmd_meter_design_t* out) { return fmd::meter_design(fs, out, &fmd::meter_global_error()); }

int fmd_meter_tp_design(int fs, fmd_meter_tp_design_t* out) { return fmd::meter_tp_design(fs, out, &fmd::meter_global_error()); }

double fmd_meter_dbtp(float peak) {
    if (peak == 0.0f) return -std::numeric_limits<double>::infinity();
    return 20.0 * std::log10((double)peak);
}

int fmd_meter_range(const unsigned* hist, const fmd_meter_design_t* d, double* lra, double* low, double* high) {
    if (!hist || !d || !lra || !low || !high) { fmd::meter_global_error() = "null histogram, design or output"; return FMD_ERR_ARG; }
    unsigned long long n0 = 0;
    double s = 0.0;
    for (int j = 0; j < fmd::kMeterBins; j++) {
        n0 += hist[j];
        s += (double)hist[j] * d->centre[j];
    }
    if (n0 == 0) { fmd::meter_global_error() = "the range histogram is empty"; return FMD_ERR_STATE; }
    const double gate = 0.01 * (s / (double)n0);
    unsigned long long n = 0;
    for (int j = 0; j < fmd::kMeterBins; j++)
        if (d->centre[j] >= gate) n += hist[j];
    if (n == 0) { fmd::meter_global_error() = "no short-term value passes the relative gate"; return FMD_ERR_STATE; }
    const unsigned long long r10 = (unsigned long long)std::floor(0.10 * (double)(n - 1) + 0.5);
    const unsigned long long r95 = (unsigned long long)std::floor(0.95 * (double)(n - 1) + 0.5);
    int j10 = -1, j95 = -1;
    unsigned long long cum = 0;
    for (int j = 0; j < fmd::kMeterBins; j++) {
        if (!(d->centre[j] >= gate)) continue;
        cum += hist[j];
        if (j10 < 0 && cum > r10) j10 = j;
        if (j95 < 0 && cum > r95) j95 = j;
    }
    *low = -70.0 + 0.1 * (double)j10 + 0.05;
    *high = -70.0 + 0.1 * (double)j95 + 0.05;
    *lra = (double)(j95 - j10) / 10.0;
    return FMD_OK;
}

double fmd_meter_lufs(double energy) {
    if (energy == 0.0) return -std::numeric_limits<double>::infinity();
    return -0.691 + 10.0 * std::log10(energy);
}

int fmd_meter_integrated(const unsigned* hist, const fmd_meter_design_t* d, double* lufs) {
    if (!hist || !d || !lufs) { fmd::meter_global_error() = "null histogram, design or output"; return FMD_ERR_ARG; }
    unsigned long long n = 0;
    double s = 0.0;
    for (int j = 0; j < fmd::kMeterBins; j++) {
        n += hist[j];
        s += (double)hist[j] * d->centre[j];
    }
    if (n == 0) { *lufs = -std::numeric_limits<double>::infinity(); return FMD_OK; }
    const double gate = 0.1 * (s / (double)n);
    unsigned long long nk = 0;
    double sk = 0.0;
    for (int j = 0; j < fmd::kMeterBins; j++) {
        if (!(d->centre[j] >= gate)) continue;
        nk += hist[j];
        sk += (double)hist[j] * d->centre[j];
    }
    *lufs = nk == 0 ? -std::numeric_limits<double>::infinity() : fmd_meter_lufs(sk / (double)nk);
    return FMD_OK;
}

int fmd_meter_momentary(const fmd_meter_status* s, double* lufs) {
    if (!s || !lufs) { fmd::meter_global_error() = "null status or output"; return FMD_ERR_ARG; }
    if (s->subblocks < 4) { fmd::meter_global_error() = "momentary loudness needs 4 completed sub-blocks"; return FMD_ERR_STATE; }
    const unsigned long long G = s->subblocks;
    const double* e = s->energy_ring;
    const int R = fmd::kMeterRing;
    *lufs = fmd_meter_lufs((((e[(G - 4) % R] + e[(G - 3) % R]) + e[(G - 2) % R]) + e[(G - 1) % R]) / 4.0);
    return FMD_OK;
}

int fmd_meter_short_term(const fmd_meter_status* s, double* lufs) {
    if (!s || !lufs) { fmd::meter_global_error() = "null status or output"; return FMD_ERR_ARG; }
    if (s->subblocks < (unsigned long long)fmd::kMeterRing) { fmd::meter_global_error() = "short-term loudness needs 30 completed sub-blocks"; return FMD_ERR_STATE; }
    double sum = 0.0;
    for (unsigned long long g = s->subblocks - fmd::kMeterRing; g < s->subblocks; g++) sum += s->energy_ring[g % fmd::kMeterRing];
    *lufs = fmd_meter_lufs(sum / 30.0);
    return FMD_OK;
}

}  // extern "C"
