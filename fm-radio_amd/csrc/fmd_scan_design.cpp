// Band scanner, host side: detection on the averaged PSD (include/fmdemod.h, "Band scan").  It runs once per query over at most 16384
// bins, in double, so it stays on the host where the CPU tests can pin it.
#include "fmd_scan_design.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <set>
#include <vector>

namespace fmd {

static constexpr double kMaxRasterPoints = 1e6;

bool scan_nfft_ok(int nfft) { return nfft >= 256 && nfft <= 16384 && (nfft & (nfft - 1)) == 0; }

std::string& scan_global_error() {
    static thread_local std::string e;
    return e;
}

static int arg_error(std::string* err, const char* msg, double v) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), msg, v);
    if (err) *err = buf;
    return FMD_ERR_ARG;
}

int scan_detect(const double* psd, int nfft, double fs_in, const fmd_scan_params* p, fmd_scan_station* out, int cap, int* n_found,
                std::string* err) {
    if (!psd || !p || !n_found || cap < 0 || (cap > 0 && !out)) return arg_error(err, "null pointer or negative capacity (%g)", cap);
    if (!scan_nfft_ok(nfft)) return arg_error(err, "nfft %g is not a power of two in 256 ... 16384", nfft);
    if (!(std::isfinite(fs_in) && fs_in > 0)) return arg_error(err, "fs_in %g must be finite and > 0", fs_in);
    if (!(std::isfinite(p->raster_hz) && p->raster_hz > 0)) return arg_error(err, "raster_hz %g must be finite and > 0", p->raster_hz);
    if (!std::isfinite(p->raster_origin_hz)) return arg_error(err, "raster_origin_hz %g must be finite", p->raster_origin_hz);
    if (!(std::isfinite(p->channel_bw_hz) && p->channel_bw_hz > 0)) return arg_error(err, "channel_bw_hz %g must be finite and > 0", p->channel_bw_hz);
    if (std::isnan(p->min_snr_db)) return arg_error(err, "min_snr_db %g must not be NaN", p->min_snr_db);
    if (!(p->usable_fraction > 0 && p->usable_fraction <= 1)) return arg_error(err, "usable_fraction %g must lie in (0, 1]", p->usable_fraction);
    if (!(p->noise_quantile >= 0 && p->noise_quantile <= 1)) return arg_error(err, "noise_quantile %g must lie in [0, 1]", p->noise_quantile);
    if (!(std::isfinite(p->min_spacing_hz) && p->min_spacing_hz >= 0)) return arg_error(err, "min_spacing_hz %g must be finite and >= 0", p->min_spacing_hz);
    const int N = nfft, h = N / 2;
    for (int i = 0; i < N; i++) {
        if (!std::isfinite(psd[i])) return arg_error(err, "the PSD is not finite (bin %g): a non-finite sample reached the scanner since its last reset", i);
        if (psd[i] < 0) return arg_error(err, "the PSD is negative at bin %g", i);
    }
    const double delta = fs_in / N, lim = p->usable_fraction * fs_in / 2;
    // noise floor: rank floor(q (m - 1)) of the usable bins, ascending
    std::vector<double> usable;
    for (int i = 0; i < N; i++)
        if (std::fabs((double)(i - h) * delta) <= lim) usable.push_back(psd[i]);
    if (usable.empty()) return arg_error(err, "usable_fraction %g leaves no usable bin", p->usable_fraction);
    const size_t rank = (size_t)std::floor(p->noise_quantile * (double)(usable.size() - 1));
    std::nth_element(usable.begin(), usable.begin() + rank, usable.end());
    const double nu = usable[rank];
    // raster points inside the usable band, each with its channel window
    struct Cand { double f, pc, snr; };
    std::vector<Cand> cands;
    const double half_bw = p->channel_bw_hz / 2;
    // the raster's index range, counted in double before any conversion to an integer
    const double j_lo_d = std::floor((-lim - p->raster_origin_hz) / p->raster_hz) - 1, j_hi_d = std::ceil((lim - p->raster_origin_hz) / p->raster_hz) + 1;
    if (!(j_hi_d - j_lo_d <= kMaxRasterPoints))
        return arg_error(err, "raster_hz %g gives more than 1000000 raster points in the usable band", p->raster_hz);
    const long long j_lo = (long long)j_lo_d, j_hi = (long long)j_hi_d;
    for (long long j = j_lo; j <= j_hi; j++) {
        const double fc = p->raster_origin_hz + (double)j * p->raster_hz;
        if (!(std::fabs(fc) + half_bw <= lim)) continue;
        // the window, clipped to the N bins: with usable_fraction = 1 a channel may end exactly at +fs_in / 2, which is bin N (no such bin:
        // it is bin 0, -fs_in / 2, already counted where the band starts)
        const long long lo = std::max(0LL, (long long)std::ceil((fc - half_bw) / delta) + h);
        const long long hi = std::min((long long)N - 1, (long long)std::floor((fc + half_bw) / delta) + h);
        if (hi < lo) continue;                                   // a channel narrower than one bin holds no bin: P_c = 0
        double sum = 0;
        for (long long i = lo; i <= hi; i++) sum += psd[i];
        const double pc = delta * sum;
        if (!(pc > 0)) continue;
        const double snr = nu > 0 ? 10 * std::log10(pc / (nu * delta * (double)(hi - lo + 1))) : std::numeric_limits<double>::infinity();
        if (snr >= p->min_snr_db) cands.push_back({fc, pc, snr});
    }
    // one detection per station: strongest first, ties to the lower offset; accept unless an accepted station is closer than min_spacing
    std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) { return a.pc != b.pc ? a.pc > b.pc : a.f < b.f; });
    // (the accepted offsets are kept sorted, so each candidate is checked against its few neighbours, not against every accepted station)
    std::vector<Cand> acc;
    std::set<double> taken;
    for (const Cand& c : cands) {
        bool near = false;
        auto it = taken.lower_bound(c.f - p->min_spacing_hz);
        if (it != taken.begin()) --it;
        for (; it != taken.end() && *it <= c.f + p->min_spacing_hz && !near; ++it) near = std::fabs(*it - c.f) < p->min_spacing_hz;
        if (!near) { acc.push_back(c); taken.insert(c.f); }
    }
    std::sort(acc.begin(), acc.end(), [](const Cand& a, const Cand& b) { return a.f < b.f; });
    const int n = (int)acc.size();
    for (int k = 0; k < n && k < cap; k++) out[k] = {acc[k].f, 10 * std::log10(acc[k].pc), acc[k].snr};
    *n_found = n;
    return FMD_OK;
}

}  // namespace fmd

extern "C" {

int fmd_scan_default_nfft(double fs_in) {
    if (!(std::isfinite(fs_in) && fs_in > 0)) return FMD_ERR_ARG;
    int n = 256;
    while (n < 16384 && fs_in / n > 5000.0) n *= 2;
    return n;
}

void fmd_scan_default_params(fmd_scan_params* p) {
    if (!p) return;
    p->raster_hz = 100e3;
    p->raster_origin_hz = 0;
    p->channel_bw_hz = 100e3;
    p->min_snr_db = 10;
    p->usable_fraction = 0.8;
    p->noise_quantile = 0.1;
    p->min_spacing_hz = 150e3;
}

int fmd_scan_detect(const double* psd, int nfft, double fs_in, const fmd_scan_params* p, fmd_scan_station* out, int cap, int* n_found) {
    return fmd::scan_detect(psd, nfft, fs_in, p, out, cap, n_found, &fmd::scan_global_error());
}

}  // extern "C"
