// Audio fault monitor, device side (include/fmdemod.h, "Audio fault monitor").
//
// NOT in the reference.  Per station and per 100 ms interval the sums LL = sum L^2, RR = sum R^2, LR = sum L R and the two rail peaks of
// the station audio [C][in_stride][2] f32 that the resampler, the mixer and the loudness meter read, read in place; at an interval's end
// the five hysteresis detectors (silence, left lost, right lost, antiphase, mono), and at a call's end the [C] flags and ok bytes.
//
// One kernel per call, k_audmon, on the row walk of fmd_rows.h (one wavefront per station, rows of 256 frames, four rows in registers
// ahead): interleaved L, R f32 has the byte layout of the carrier squelch's cf32.  With NP = 64 and j = (r >> 2) & 63 lane l owns exactly
// partial l of each of the three sums and adds its four terms of a row in ascending r; a frame that reads as (+0, +0) changes no partial
// (fma(+0, +0, s) = s: a partial is never -0) and no peak.  At an interval's end the partials fold by cross-lane moves in the contract's
// halving order, and lane 0 alone writes the ring, runs the detectors on the station's record and stores, with ordinary stores.  The open
// interval's 1.5 KB of partials are read at the call's start and written at its end.  No atomics, no LDS, no scratch.
//
// Denormals: fp64 and fp32 denormals are kept (hipcc's default mode; this file is NOT built with -fgpu-flush-denormals-to-zero).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fmd_audmon_design.h"
#include "fmd_rows.h"
#include "fmd_side.h"
#include "fmdemod.h"

using fmd::AudmonGate;
using fmd::kAudmonDetectors;
using fmd::kAudmonPartials;
using fmd::kAudmonRing;

namespace {

namespace rows = fmd::rows;
using rows::kQ;                      // frames per lane and row
using rows::kT;                      // threads per workgroup: one wavefront, one station
constexpr int kPf = 4;               // rows loaded ahead
constexpr int kPartD = 3 * kAudmonPartials;    // doubles per station: the open interval's ll, rr and lr partials
static_assert(kAudmonPartials == kT && kAudmonRing == 30 && kAudmonDetectors == 5, "k_audmon's lane layout");

static_assert(sizeof(fmd_audmon_status) == 840 && offsetof(fmd_audmon_status, intervals) == 8 && offsetof(fmd_audmon_status, intervals_flagged) == 16 &&
              offsetof(fmd_audmon_status, ring_ll) == 56 && offsetof(fmd_audmon_status, ring_rr) == 296 && offsetof(fmd_audmon_status, ring_lr) == 536 &&
              offsetof(fmd_audmon_status, last_peak) == 776 && offsetof(fmd_audmon_status, hold_peak) == 784 && offsetof(fmd_audmon_status, run) == 792 &&
              offsetof(fmd_audmon_status, transitions) == 812 && offsetof(fmd_audmon_status, nonfinite) == 832 && offsetof(fmd_audmon_status, flags) == 836 &&
              offsetof(fmd_audmon_status, ok) == 837 && offsetof(fmd_audmon_status, reserved) == 838, "fmd_audmon_status layout");
static_assert(sizeof(AudmonGate) == 80 && sizeof(fmd_audmon_params) == 80, "AudmonGate and fmd_audmon_params layout");

// in [C][in_stride] frames (L, R); gate [C]; status [C]; part [C][3][64]; carry [C][2]; out_flags, out_ok [C] or null
__global__ __launch_bounds__(kT) void k_audmon(const float2* __restrict__ in, long long in_stride, long long n, const uint8_t* __restrict__ active, int M,
                                               const AudmonGate* __restrict__ gate, fmd_audmon_status* __restrict__ status, double* __restrict__ part,
                                               float* __restrict__ carry, uint8_t* __restrict__ out_flags, uint8_t* __restrict__ out_ok) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (active && active[c] == 0) return;                                    // (uniform over the wavefront)
    fmd_audmon_status* st = status + c;
    const AudmonGate gt = gate[c];                                           // (uniform: read once)
    unsigned flags = st->flags;
    if (n == 0) {                                                            // nothing of the station changes but its bytes, which are still written
        if (lane == 0) {
            const uint8_t ok = (uint8_t)((flags & gt.alarm_mask) == 0);
            st->ok = ok;
            if (out_flags) out_flags[c] = (uint8_t)flags;
            if (out_ok) out_ok[c] = ok;
        }
        return;
    }
    const float2* base = in + (size_t)c * (size_t)in_stride;
    double* pp = part + (size_t)c * kPartD + lane;

    const unsigned long long frames0 = st->frames;
    unsigned long long G = st->intervals;
    const int r0 = __builtin_amdgcn_readfirstlane((int)(frames0 - G * (unsigned long long)M));   // the first frame's place in its interval
    float cpl = carry[2 * c], cpr = carry[2 * c + 1];                        // the open interval's peaks before this call
    double ll = pp[0], rr = pp[kAudmonPartials], lr = pp[2 * kAudmonPartials];
    float pl = 0.0f, pr = 0.0f;                                              // the lane's, over the segment at hand
    float hl = 0.0f, hr = 0.0f;                                              // over the call

    rows::walk<kPf>(base, lane, n, M, r0, make_float2(0.0f, 0.0f),
        [&](const float2 (&v)[kQ]) {
#pragma unroll
            for (int k = 0; k < kQ; k++) {
                const double l = (double)v[k].x, r_ = (double)v[k].y;
                ll = fma(l, l, ll);
                rr = fma(r_, r_, rr);
                lr = fma(l, r_, lr);
                pl = fmaxf(pl, fabsf(v[k].x));
                pr = fmaxf(pr, fabsf(v[k].y));
            }
        },
        [&](bool complete) {
            pl = rows::wave_max(pl); pr = rows::wave_max(pr);      // the segment's peaks
            cpl = fmaxf(cpl, pl); cpr = fmaxf(cpr, pr);
            hl = fmaxf(hl, pl); hr = fmaxf(hr, pr);
            pl = 0.0f; pr = 0.0f;
            if (!complete) return;
            rows::fold(ll, rr, lr);
            if (lane == 0) {
                const double LL = ll, RR = rr, LR = lr;
                const int k = (int)(G % (unsigned long long)kAudmonRing);
                st->ring_ll[k] = LL; st->ring_rr[k] = RR; st->ring_lr[k] = LR;
                st->last_peak[0] = cpl; st->last_peak[1] = cpr;
                const bool finite = rows::finite(LL) && rows::finite(RR) && rows::finite(LR);
                if (!finite) st->nonfinite++;
                const double E = LL + RR;
                const bool silent = !(finite && E > gt.min_e);
                auto detect = [&](int d, bool bad) {
                    flags = rows::detect(flags, d, bad, gt.raise_intervals[d], gt.clear_intervals[d], st->run[d], st->transitions[d]);
                };
                detect(0, silent);
                if (!silent) {                                               // (silent: detectors 1 ... 4 hold)
                    const double c_loss = gt.c_loss;
                    const double S = fma(-2.0, LR, E), Md = fma(2.0, LR, E);
                    detect(1, LL < c_loss * RR);
                    detect(2, RR < c_loss * LL);
                    detect(3, LR < 0.0 && LR * LR > gt.c_anti * (LL * RR));
                    detect(4, S < gt.c_mono * Md);
                }
#pragma unroll
                for (int d = 0; d < kAudmonDetectors; d++)
                    if (flags & (1u << d)) st->intervals_flagged[d]++;
            }
            G++;
            ll = 0.0; rr = 0.0; lr = 0.0;
            cpl = 0.0f; cpr = 0.0f;
        });

    // what the next call needs: the open interval's partials and peaks, and the record
    pp[0] = ll; pp[kAudmonPartials] = rr; pp[2 * kAudmonPartials] = lr;
    if (lane == 0) {
        carry[2 * c] = cpl; carry[2 * c + 1] = cpr;
        st->hold_peak[0] = fmaxf(st->hold_peak[0], hl);
        st->hold_peak[1] = fmaxf(st->hold_peak[1], hr);
        st->frames = frames0 + (unsigned long long)n;
        st->intervals = G;
        const uint8_t ok = (uint8_t)((flags & gt.alarm_mask) == 0);
        st->flags = (unsigned char)flags;
        st->ok = ok;
        if (out_flags) out_flags[c] = (uint8_t)flags;
        if (out_ok) out_ok[c] = ok;
    }
}

// stations c0 ... as after create (everything 0, every flag clear, ok = 1), or with `peaks` their hold_peak alone
__global__ __launch_bounds__(kT) void k_audmon_reset(int c0, int peaks, fmd_audmon_status* __restrict__ status, double* __restrict__ part, float* __restrict__ carry) {
    const int c = c0 + blockIdx.x, t = threadIdx.x;
    fmd_audmon_status* st = status + c;
    if (peaks) {
        if (t == 0) { st->hold_peak[0] = 0.0f; st->hold_peak[1] = 0.0f; }
        return;
    }
    unsigned* w = reinterpret_cast<unsigned*>(st);
    for (int i = t; i < (int)(sizeof(fmd_audmon_status) / 4); i += kT) w[i] = 0u;
    for (int i = t; i < kPartD; i += kT) part[(size_t)c * kPartD + i] = 0.0;
    __syncthreads();
    if (t == 0) { carry[2 * c] = 0.0f; carry[2 * c + 1] = 0.0f; st->ok = 1; }
}

// the parameters of stations c0 ...
__global__ __launch_bounds__(kT) void k_audmon_set(int c0, int cn, AudmonGate g, AudmonGate* __restrict__ gate, fmd_audmon_status* __restrict__ status) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= cn) return;
    gate[c0 + i] = g;
    status[c0 + i].ok = (unsigned char)((status[c0 + i].flags & g.alarm_mask) == 0);
}

}  // namespace

struct fmd_audmon_s {
    int C = 0, fs = 0, M = 0;
    long long max_in = 0;
    std::vector<fmd_audmon_params> params;   // [C], as set
    fmd_audmon_status* d_status = nullptr;   // [C]
    AudmonGate* d_gate = nullptr;            // [C]
    double* d_part = nullptr;                // [C][3][64]
    float* d_carry = nullptr;                // [C][2]
    fmd::CallOrder order;                    // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int am_fail(fmd_audmon a, int code, const char* fmt, A... args) { return fmd::fail(a ? a->err : fmd::audmon_global_error(), code, fmt, args...); }

static int am_reset(fmd_audmon a, int channel, int peaks) {
    if (!a) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, a->C, &c0, &cn)) return am_fail(a, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, a->C);
    if (!a->order.quiesce()) return am_fail(a, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_audmon_reset, dim3((unsigned)cn), dim3(kT), 0, nullptr, c0, peaks, a->d_status, a->d_part, a->d_carry);
    if (const char* e = fmd::control_end("k_audmon_reset launch failed")) return am_fail(a, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

extern "C" {

int fmd_audmon_create(const fmd_audmon_config* cfg, fmd_audmon* out) {
    if (!cfg || !out) return am_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->n_channels <= 0 || cfg->max_input_frames <= 0 || cfg->max_input_frames > (1LL << 30))
        return am_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_frames %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_frames);
    const int M = fmd::audmon_interval(cfg->fs);
    if (M == 0) return am_fail(nullptr, FMD_ERR_ARG, "fs %d is not a multiple of 10 in 8000 ... 192000", cfg->fs);
    if (fmd_device_count() <= 0) return am_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return am_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_audmon a = new fmd_audmon_s();
    a->C = cfg->n_channels; a->fs = cfg->fs; a->M = M; a->max_in = cfg->max_input_frames;
    fmd_audmon_params p{};
    fmd_audmon_default_params(&p);
    a->params.assign((size_t)a->C, p);
    const size_t C = (size_t)a->C;
    bool ok = a->order.init(dev);
    ok = ok && hipMalloc(&a->d_status, sizeof(fmd_audmon_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&a->d_gate, sizeof(AudmonGate) * C) == hipSuccess;
    ok = ok && hipMalloc(&a->d_part, sizeof(double) * kPartD * C) == hipSuccess;
    ok = ok && hipMalloc(&a->d_carry, sizeof(float) * 2 * C) == hipSuccess;
    // (the reset first: set_params reads the record's flags)
    if (!ok || fmd_audmon_reset(a, -1) != FMD_OK || fmd_audmon_set_params(a, -1, &p) != FMD_OK) {
        fmd_audmon_destroy(a);
        return am_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed");
    }
    *out = a;
    return FMD_OK;
}

int fmd_audmon_destroy(fmd_audmon a) {
    if (!a) return FMD_ERR_ARG;
    (void)a->order.quiesce();
    for (void* p : {(void*)a->d_status, (void*)a->d_gate, (void*)a->d_part, (void*)a->d_carry})
        if (p) (void)hipFree(p);
    delete a;
    return FMD_OK;
}

int fmd_audmon_reset(fmd_audmon a, int channel) { return am_reset(a, channel, 0); }

int fmd_audmon_reset_peaks(fmd_audmon a, int channel) { return am_reset(a, channel, 1); }

int fmd_audmon_set_params(fmd_audmon a, int channel, const fmd_audmon_params* p) {
    if (!a) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, a->C, &c0, &cn)) return am_fail(a, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, a->C);
    AudmonGate g;
    if (fmd::audmon_gate(p, a->M, &g, &a->err) != FMD_OK) return FMD_ERR_ARG;
    if (!a->order.quiesce()) return am_fail(a, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_audmon_set, dim3((unsigned)((cn + kT - 1) / kT)), dim3(kT), 0, nullptr, c0, cn, g, a->d_gate, a->d_status);
    if (const char* e = fmd::control_end("k_audmon_set launch failed")) return am_fail(a, FMD_ERR_DEVICE, "%s", e);
    for (int c = c0; c < c0 + cn; c++) a->params[(size_t)c] = *p;
    return FMD_OK;
}

int fmd_audmon_get_params(fmd_audmon a, int channel, fmd_audmon_params* p) {
    if (!a || !p) return am_fail(a, FMD_ERR_ARG, "null monitor or output");
    if (channel < 0 || channel >= a->C) return am_fail(a, FMD_ERR_ARG, "channel %d outside [0, %d)", channel, a->C);
    *p = a->params[(size_t)channel];
    return FMD_OK;
}

int fmd_audmon_process_f32_dev(fmd_audmon a, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_flags, uint8_t* d_ok,
                               void* stream) {
    if (!a) return FMD_ERR_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return am_fail(a, FMD_ERR_ARG, "null input, or input not aligned to 8 bytes");
    if (n < 0 || n > in_stride || n > a->max_in)
        return am_fail(a, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or above max_input_frames %lld", n, in_stride, a->max_in);
    if (n == 0 && !d_flags && !d_ok) return FMD_OK;                          // nothing of any station changes and there is no byte to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* e = a->order.begin(s)) return am_fail(a, FMD_ERR_DEVICE, "%s", e);
    hipLaunchKernelGGL(k_audmon, dim3((unsigned)a->C), dim3(kT), 0, s, reinterpret_cast<const float2*>(d_in), in_stride, n, d_active, a->M, a->d_gate,
                       a->d_status, a->d_part, a->d_carry, d_flags, d_ok);
    if (hipGetLastError() != hipSuccess) return am_fail(a, FMD_ERR_DEVICE, "k_audmon launch failed");
    if (const char* e = a->order.end(s)) return am_fail(a, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_audmon_get_status(fmd_audmon a, fmd_audmon_status* out) {
    if (!a || !out) return am_fail(a, FMD_ERR_ARG, "null monitor or output");
    if (!a->order.quiesce()) return am_fail(a, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, a->d_status, sizeof(fmd_audmon_status) * (size_t)a->C, hipMemcpyDeviceToHost) != hipSuccess) return am_fail(a, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_audmon_status_dev(fmd_audmon a, const fmd_audmon_status** d_status) {
    if (!a || !d_status) return am_fail(a, FMD_ERR_ARG, "null monitor or output");
    *d_status = a->d_status;
    return FMD_OK;
}

const char* fmd_audmon_last_error(fmd_audmon a) { return a ? a->err.c_str() : fmd::audmon_global_error().c_str(); }

}  // extern "C"
