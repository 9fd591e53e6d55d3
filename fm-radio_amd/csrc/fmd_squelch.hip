// Carrier squelch, device side (include/fmdemod.h, "Carrier squelch").
//
// NOT in the reference.  Per station and per 50 ms interval the power moments S2 = sum |z|^2 and S4 = sum |z|^4 and the peak of the
// station baseband [C][in_stride][2] (cf32 or u8) that the demodulator takes and the channeliser writes, read in place; at an interval's
// end the hysteresis gate, and at a call's end the [C] mask byte that the other side objects take as d_active.
//
// One kernel per call, k_squelch<format>, on the row walk of fmd_rows.h (one wavefront per station, rows of 256 samples: 2 KB of cf32,
// 512 bytes of u8; four rows in registers ahead).  Lane l owns partials 4 l ... 4 l + 3 of the two interval sums outright and adds its
// terms in ascending r, r the sample's place in its interval; a sample that reads as (+0, +0) changes no partial (p = +0, s + +0 = s,
// fma(+0, +0, s) = s: a partial is never -0) and no peak.  At an interval's end the partials fold by cross-lane moves in the contract's
// halving order, and lane 0 alone runs the gate and stores, with ordinary stores.  The open interval's 4 KB of partials are read at the
// call's start and written at its end.  No atomics, no LDS, no scratch.
//
// Denormals: fp64 and fp32 denormals are kept (hipcc's default mode; this file is NOT built with -fgpu-flush-denormals-to-zero).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fmd_iq.h"
#include "fmd_rows.h"
#include "fmd_side.h"
#include "fmd_squelch_design.h"
#include "fmdemod.h"

using fmd::kSquelchPartials;
using fmd::kSquelchRing;
using fmd::SquelchGate;

namespace {

namespace rows = fmd::rows;
using rows::kQ;                      // samples (and partials) per lane and row
using rows::kRow;                    // samples per row
using rows::kT;                      // threads per workgroup: one wavefront, one station
constexpr int kPf = 4;               // rows loaded ahead
constexpr int kPartD = 2 * kSquelchPartials;   // doubles per station: the open interval's s2 and s4 partials
static_assert(kSquelchPartials == kRow && kSquelchRing == 20, "k_squelch's lane layout");

static_assert(sizeof(fmd_squelch_status) == 368 && offsetof(fmd_squelch_status, intervals) == 8 && offsetof(fmd_squelch_status, intervals_open) == 16 &&
              offsetof(fmd_squelch_status, ring_s2) == 24 && offsetof(fmd_squelch_status, ring_s4) == 184 && offsetof(fmd_squelch_status, last_peak) == 344 &&
              offsetof(fmd_squelch_status, hold_peak) == 348 && offsetof(fmd_squelch_status, run) == 352 && offsetof(fmd_squelch_status, transitions) == 356 &&
              offsetof(fmd_squelch_status, nonfinite) == 360 && offsetof(fmd_squelch_status, open) == 364 && offsetof(fmd_squelch_status, mode) == 365 &&
              offsetof(fmd_squelch_status, reserved) == 366, "fmd_squelch_status layout");
static_assert(sizeof(SquelchGate) == 40, "SquelchGate layout");

// in [C][in_stride] IQ pairs; gate [C]; status [C]; part [C][2][256]; carry [C]; mask [C] or null
template <typename S>
__global__ __launch_bounds__(kT) void k_squelch(const typename fmd::Iq<S>::raw* __restrict__ in, long long in_stride, long long n,
                                                const uint8_t* __restrict__ active, int M, const SquelchGate* __restrict__ gate,
                                                fmd_squelch_status* __restrict__ status, double* __restrict__ part, float* __restrict__ carry,
                                                uint8_t* __restrict__ mask) {
    using raw = typename fmd::Iq<S>::raw;
    const int c = blockIdx.x, lane = threadIdx.x;
    if (active && active[c] == 0) return;                                    // (uniform over the wavefront)
    fmd_squelch_status* st = status + c;
    const SquelchGate gt = gate[c];
    unsigned open = st->open;
    if (n == 0) {                                                            // nothing of the station changes; its mask byte is still written
        if (lane == 0 && mask) mask[c] = (uint8_t)(gt.mode == FMD_SQUELCH_AUTO ? open : gt.mode == FMD_SQUELCH_FORCE_OPEN);
        return;
    }
    const raw* base = in + (size_t)c * (size_t)in_stride;
    double* pp = part + (size_t)c * kPartD + kQ * lane;

    const unsigned long long samples0 = st->samples;
    unsigned long long G = st->intervals;
    const int r0 = __builtin_amdgcn_readfirstlane((int)(samples0 - G * (unsigned long long)M));   // the first sample's place in its interval
    // the gate's state: lane 0's copies are the ones that are updated and stored
    unsigned run = st->run, transitions = st->transitions, nonfinite = st->nonfinite;
    unsigned long long g_open = st->intervals_open;
    float cpk = carry[c];                                                    // the open interval's peak before this call
    double s2[kQ], s4[kQ];
#pragma unroll
    for (int k = 0; k < kQ; k++) { s2[k] = pp[k]; s4[k] = pp[kSquelchPartials + k]; }
    float pk = 0.0f;                                                         // the lane's, over the segment at hand
    float hmax = 0.0f;                                                       // over the call

    rows::walk<kPf>(base, lane, n, M, r0, fmd::Iq<S>::zero(),
        [&](const raw (&v)[kQ]) {
#pragma unroll
            for (int k = 0; k < kQ; k++) {
                const float2 z = fmd::Iq<S>::cf32(v[k]);
                const double I = (double)z.x, Q = (double)z.y;
                const double p = fma(I, I, Q * Q);
                s2[k] = s2[k] + p;
                s4[k] = fma(p, p, s4[k]);
                pk = fmaxf(pk, fmaxf(fabsf(z.x), fabsf(z.y)));
            }
        },
        [&](bool complete) {
            pk = rows::wave_max(pk);                                         // the segment's peak
            cpk = fmaxf(cpk, pk);
            hmax = fmaxf(hmax, pk);
            pk = 0.0f;
            if (!complete) return;
#pragma unroll
            for (int k = 0; k < kQ; k++) rows::fold(s2[k], s4[k]);           // w = 128 ... 4: partial j + w sits 'w / 4' lanes up, so each of
                                                                             // the lane's four partials folds across lanes on a chain of its own
            s2[0] += s2[2]; s2[1] += s2[3]; s2[0] += s2[1];                  // w = 2, 1
            s4[0] += s4[2]; s4[1] += s4[3]; s4[0] += s4[1];
            if (lane == 0) {
                const double S2 = s2[0], S4 = s4[0];
                const int k = (int)(G % (unsigned long long)kSquelchRing);
                st->ring_s2[k] = S2; st->ring_s4[k] = S4; st->last_peak = cpk;
                const bool finite = rows::finite(S2) && rows::finite(S4);
                if (!finite) nonfinite++;
                const double a = S2 * S2;
                const double d = fma(-(double)M, S4, 2.0 * a);
                const bool level = finite && S2 >= gt.min_s2;
                if (!open) {
                    run = level && d > gt.c_open * a ? run + 1 : 0;
                    if (run >= (unsigned)gt.open_intervals) { open = 1; run = 0; transitions++; }
                } else {
                    run = level && d > gt.c_close * a ? 0 : run + 1;
                    if (run >= (unsigned)gt.close_intervals) { open = 0; run = 0; transitions++; }
                }
                if (open) g_open++;
            }
            G++;
#pragma unroll
            for (int k = 0; k < kQ; k++) { s2[k] = 0.0; s4[k] = 0.0; }
            cpk = 0.0f;
        });

    // what the next call needs: the open interval's partials and peak, and the gate
#pragma unroll
    for (int k = 0; k < kQ; k++) { pp[k] = s2[k]; pp[kSquelchPartials + k] = s4[k]; }
    if (lane == 0) {
        carry[c] = cpk;
        st->hold_peak = fmaxf(st->hold_peak, hmax);
        st->samples = samples0 + (unsigned long long)n;
        st->intervals = G;
        st->intervals_open = g_open;
        st->run = run; st->transitions = transitions; st->nonfinite = nonfinite;
        st->open = (unsigned char)open;
        if (mask) mask[c] = (uint8_t)(gt.mode == FMD_SQUELCH_AUTO ? open : gt.mode == FMD_SQUELCH_FORCE_OPEN);
    }
}

// stations c0 ... as after create (everything 0, the gate closed, the mode the parameters'), or with `peaks` their hold_peak alone
__global__ __launch_bounds__(kT) void k_squelch_reset(int c0, int peaks, const SquelchGate* __restrict__ gate, fmd_squelch_status* __restrict__ status,
                                                      double* __restrict__ part, float* __restrict__ carry) {
    const int c = c0 + blockIdx.x, t = threadIdx.x;
    fmd_squelch_status* st = status + c;
    if (peaks) {
        if (t == 0) st->hold_peak = 0.0f;
        return;
    }
    unsigned* w = reinterpret_cast<unsigned*>(st);
    for (int i = t; i < (int)(sizeof(fmd_squelch_status) / 4); i += kT) w[i] = 0u;
    for (int i = t; i < kPartD; i += kT) part[(size_t)c * kPartD + i] = 0.0;
    __syncthreads();
    if (t == 0) { carry[c] = 0.0f; st->mode = (unsigned char)gate[c].mode; }
}

// the parameters of stations c0 ...
__global__ __launch_bounds__(kT) void k_squelch_set(int c0, int cn, SquelchGate g, SquelchGate* __restrict__ gate, fmd_squelch_status* __restrict__ status) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= cn) return;
    gate[c0 + i] = g;
    status[c0 + i].mode = (unsigned char)g.mode;
}

}  // namespace

struct fmd_squelch_s {
    int C = 0, fs = 0, M = 0;
    long long max_in = 0;
    std::vector<fmd_squelch_params> params;  // [C], as set
    fmd_squelch_status* d_status = nullptr;  // [C]
    SquelchGate* d_gate = nullptr;           // [C]
    double* d_part = nullptr;                // [C][2][256]
    float* d_carry = nullptr;                // [C]
    fmd::CallOrder order;                    // behind the previous call's work
    std::string err;
};

template <typename... A>
static int sq_fail(fmd_squelch q, int code, const char* fmt, A... args) { return fmd::fail(q ? q->err : fmd::squelch_global_error(), code, fmt, args...); }

static int sq_reset(fmd_squelch q, int channel, int peaks) {
    if (!q) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, q->C, &c0, &cn)) return sq_fail(q, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, q->C);
    if (!q->order.quiesce()) return sq_fail(q, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_squelch_reset, dim3((unsigned)cn), dim3(kT), 0, nullptr, c0, peaks, q->d_gate, q->d_status, q->d_part, q->d_carry);
    if (const char* e = fmd::control_end("k_squelch_reset launch failed")) return sq_fail(q, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

template <typename S>
static int sq_process(fmd_squelch q, const void* d_in, size_t align, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_mask, void* stream) {
    if (!q) return FMD_ERR_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % align != 0) return sq_fail(q, FMD_ERR_ARG, "null input, or input not aligned to %zu bytes", align);
    if (n < 0 || n > in_stride || n > q->max_in)
        return sq_fail(q, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or above max_input_samples %lld", n, in_stride, q->max_in);
    if (n == 0 && !d_mask) return FMD_OK;                                    // nothing of any station changes and there is no mask to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const char* e = q->order.begin(s)) return sq_fail(q, FMD_ERR_DEVICE, "%s", e);   // every station's state carries over from call to call
    hipLaunchKernelGGL(k_squelch<S>, dim3((unsigned)q->C), dim3(kT), 0, s, static_cast<const typename fmd::Iq<S>::raw*>(d_in), in_stride, n, d_active, q->M,
                       q->d_gate, q->d_status, q->d_part, q->d_carry, d_mask);
    if (hipGetLastError() != hipSuccess) return sq_fail(q, FMD_ERR_DEVICE, "k_squelch launch failed");
    if (const char* e = q->order.end(s)) return sq_fail(q, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

extern "C" {

int fmd_squelch_create(const fmd_squelch_config* cfg, fmd_squelch* out) {
    if (!cfg || !out) return sq_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->n_channels <= 0 || cfg->max_input_samples <= 0 || cfg->max_input_samples > (1LL << 30))
        return sq_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_samples %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_samples);
    const int M = fmd::squelch_interval(cfg->fs);
    if (M == 0) return sq_fail(nullptr, FMD_ERR_ARG, "fs %d is not a multiple of 1000 in 192000 ... 384000", cfg->fs);
    if (fmd_device_count() <= 0) return sq_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return sq_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_squelch q = new fmd_squelch_s();
    q->C = cfg->n_channels; q->fs = cfg->fs; q->M = M; q->max_in = cfg->max_input_samples;
    fmd_squelch_params p{};
    fmd_squelch_default_params(&p);
    q->params.assign((size_t)q->C, p);
    const size_t C = (size_t)q->C;
    bool ok = q->order.init(dev);
    ok = ok && hipMalloc(&q->d_status, sizeof(fmd_squelch_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&q->d_gate, sizeof(SquelchGate) * C) == hipSuccess;
    ok = ok && hipMalloc(&q->d_part, sizeof(double) * kPartD * C) == hipSuccess;
    ok = ok && hipMalloc(&q->d_carry, sizeof(float) * C) == hipSuccess;
    if (!ok || fmd_squelch_set_params(q, -1, &p) != FMD_OK || fmd_squelch_reset(q, -1) != FMD_OK) {
        fmd_squelch_destroy(q);
        return sq_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed");
    }
    *out = q;
    return FMD_OK;
}

int fmd_squelch_destroy(fmd_squelch q) {
    if (!q) return FMD_ERR_ARG;
    (void)q->order.quiesce();
    for (void* p : {(void*)q->d_status, (void*)q->d_gate, (void*)q->d_part, (void*)q->d_carry})
        if (p) (void)hipFree(p);
    delete q;
    return FMD_OK;
}

int fmd_squelch_reset(fmd_squelch q, int channel) { return sq_reset(q, channel, 0); }

int fmd_squelch_reset_peaks(fmd_squelch q, int channel) { return sq_reset(q, channel, 1); }

int fmd_squelch_set_params(fmd_squelch q, int channel, const fmd_squelch_params* p) {
    if (!q) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, q->C, &c0, &cn)) return sq_fail(q, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, q->C);
    SquelchGate g;
    if (fmd::squelch_gate(p, q->M, &g, &q->err) != FMD_OK) return FMD_ERR_ARG;
    if (!q->order.quiesce()) return sq_fail(q, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_squelch_set, dim3((unsigned)((cn + kT - 1) / kT)), dim3(kT), 0, nullptr, c0, cn, g, q->d_gate, q->d_status);
    if (const char* e = fmd::control_end("k_squelch_set launch failed")) return sq_fail(q, FMD_ERR_DEVICE, "%s", e);
    for (int c = c0; c < c0 + cn; c++) q->params[(size_t)c] = *p;
    return FMD_OK;
}

int fmd_squelch_get_params(fmd_squelch q, int channel, fmd_squelch_params* p) {
    if (!q || !p) return sq_fail(q, FMD_ERR_ARG, "null squelch or output");
    if (channel < 0 || channel >= q->C) return sq_fail(q, FMD_ERR_ARG, "channel %d outside [0, %d)", channel, q->C);
    *p = q->params[(size_t)channel];
    return FMD_OK;
}

int fmd_squelch_process_cf32_dev(fmd_squelch q, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_mask, void* stream) {
    return sq_process<float2>(q, d_in, 8, in_stride, n, d_active, d_mask, stream);
}

int fmd_squelch_process_u8_dev(fmd_squelch q, const uint8_t* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_mask, void* stream) {
    return sq_process<uint8_t>(q, d_in, 2, in_stride, n, d_active, d_mask, stream);
}

int fmd_squelch_get_status(fmd_squelch q, fmd_squelch_status* out) {
    if (!q || !out) return sq_fail(q, FMD_ERR_ARG, "null squelch or output");
    if (!q->order.quiesce()) return sq_fail(q, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, q->d_status, sizeof(fmd_squelch_status) * (size_t)q->C, hipMemcpyDeviceToHost) != hipSuccess) return sq_fail(q, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_squelch_status_dev(fmd_squelch q, const fmd_squelch_status** d_status) {
    if (!q || !d_status) return sq_fail(q, FMD_ERR_ARG, "null squelch or output");
    *d_status = q->d_status;
    return FMD_OK;
}

const char* fmd_squelch_last_error(fmd_squelch q) { return q ? q->err.c_str() : fmd::squelch_global_error().c_str(); }

}  // extern "C"
