// The limiter's design, defaults, loudness helper and parameter checks: the pure functions that tests/test_limiter_cpu.py holds to the
// header's formulas.
#include "fmd_limiter_design.h"

#include <cmath>
#include <cstdio>

namespace fmd {

std::string& limiter_global_error() {
    thread_local std::string e;
    return e;
}

int limiter_check_call(int C, long long max_in, const void* d_in, long long in_stride, long long n, const void* d_out, long long out_stride, std::string* err) {
    char buf[256];
    auto no = [&](const char* fmt, long long a, long long b) { snprintf(buf, sizeof(buf), fmt, a, b); *err = buf; return FMD_ERR_ARG; };
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return no("null input, or input not aligned to 8 bytes", 0, 0);
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 8 != 0) return no("null output, or output not aligned to 8 bytes", 0, 0);
    if (n < 0 || n > in_stride) return no("n %lld outside [0, in_stride %lld]", n, in_stride);
    if (n > out_stride) return no("n %lld above out_stride %lld", n, out_stride);
    if (n > max_in) return no("n %lld above max_input_frames %lld", n, max_in);
    if (n > 0) {                                                             // the bytes the call reads and the bytes it may write
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(d_in), a1 = a0 + 8u * (uintptr_t)((long long)(C - 1) * in_stride + n);
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(d_out), b1 = b0 + 8u * (uintptr_t)((long long)(C - 1) * out_stride + n);
        if (a0 < b1 && b0 < a1) return no("the output's rows overlap the input's", 0, 0);
    }
    return FMD_OK;
}

}  // namespace fmd

static int lim_fail(int code, const char* msg) {
    fmd::limiter_global_error() = msg;
    return code;
}

extern "C" {

int fmd_limiter_design(int fs, double lookahead_ms, double release_ms, double ceiling_db, fmd_limiter_design_t* out) {
    if (!out) return lim_fail(FMD_ERR_ARG, "null output");
    if (fs < 8000 || fs > 192000) return lim_fail(FMD_ERR_ARG, "fs outside 8000 ... 192000");
    if (!(lookahead_ms >= 0.0) || !(lookahead_ms <= 1000.0)) return lim_fail(FMD_ERR_ARG, "lookahead_ms is negative, above 1000 or not a number");
    if (!(release_ms >= 0.0) || !(release_ms <= 1e12)) return lim_fail(FMD_ERR_ARG, "release_ms is negative, above 1e12 or not a number");
    if (!(ceiling_db >= -40.0) || !(ceiling_db <= 0.0)) return lim_fail(FMD_ERR_ARG, "ceiling_db outside [-40, 0]");
    const long long D = std::llround(lookahead_ms * (double)fs / 1000.0);
    if (D < 0 || D > fmd::kLimiterMaxD) return lim_fail(FMD_ERR_ARG, "the look-ahead is more than 255 frames");
    const double one = (double)fmd::kLimiterOne, frames = release_ms * (double)fs / 1000.0;
    long long step = (long long)fmd::kLimiterOne;                            // release_ms = 0: an instant release
    if (frames > 0.0) {
        const double s = one / frames;
        step = s >= one ? (long long)fmd::kLimiterOne : std::llround(s);
    }
    step = step < 1 ? 1 : step > (long long)fmd::kLimiterOne ? (long long)fmd::kLimiterOne : step;
    out->lookahead_frames = (int)D;
    out->step = (unsigned)step;
    out->ceiling = (float)std::pow(10.0, ceiling_db / 20.0);
    out->latency_frames = (int)D;
    return FMD_OK;
}

int fmd_limiter_default_config(int fs, fmd_limiter_config* cfg) {
    if (!cfg) return lim_fail(FMD_ERR_ARG, "null configuration");
    if (fs < 8000 || fs > 192000) return lim_fail(FMD_ERR_ARG, "fs outside 8000 ... 192000");
    cfg->n_channels = 1;
    cfg->fs = fs;
    cfg->lookahead_ms = 1.5;
    cfg->release_ms = 500.0;
    cfg->ceiling_db = -1.0;
    cfg->max_input_frames = 1LL << 16;
    cfg->device = -1;
    return FMD_OK;
}

float fmd_limiter_gain_for_loudness(double lufs, double target_lufs) { return (float)std::pow(10.0, (target_lufs - lufs) / 20.0); }

}  // extern "C"
