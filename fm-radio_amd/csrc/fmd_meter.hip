// Batched loudness meter, device side (include/fmdemod.h, "Batched loudness meter").
//
// NOT in the reference.  ITU-R BS.1770 K-weighting (two biquads in fp64), 100 ms sub-block energies, the 400 ms gating blocks' histogram
// and the sample peak of every station's audio, read in place from the device array the resampler and the mixer read.
//
// One kernel per call, k_meter.  The recurrences are serial in time, so the parallelism is (station x rail): one lane per rail, L and R of
// a station in adjacent lanes, 32 stations per workgroup of one wavefront.  The even lane owns the station: at a sub-block's end it takes
// the odd lane's sum by one cross-lane move and alone writes the station's ring, histogram bin and counters, with ordinary stores.  A
// station's frames are contiguous in memory, so lanes do not stride through HBM: the wavefront loads 64 frames of one station per
// instruction (8 bytes a lane), 32 stations a tile, holds the next tile in registers while it runs the current one, and hands the tile to
// the lanes through LDS, de-interleaved ([station][rail][frame], rows padded to 68 floats), from where each lane reads four of its rail's
// samples per ds_read_b128.  Per frame the dependent path is the two fmas of each biquad's first state (fma(pb1, v, s2) and pb2 * v do not
// depend on o1).  Sub-block ends fall at a different frame in every station (each counts its own frames), so they are a lane-divergent
// branch taken once in Nsb frames.
//
// Denormals: fp64 denormals are kept (hipcc's default mode; this file is NOT built with -fgpu-flush-denormals-to-zero).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "fmd_meter_design.h"
#include "fmdemod.h"

using fmd::kMeterBins;
using fmd::kMeterRing;

namespace {

constexpr int kT = 64;               // threads per workgroup: one wavefront
constexpr int kCh = kT / 2;          // stations per workgroup
constexpr int kTile = 64;            // frames per tile: one 8-byte load per lane and station
constexpr int kRow = kTile + 4;      // floats per LDS row (a row per lane; +4 keeps the 16-byte reads of 16 lanes on distinct banks)
constexpr int kCarry = 5;            // s1, s2, t1, t2, acc per (station, rail)

static_assert(sizeof(fmd_meter_status) == 280 && offsetof(fmd_meter_status, energy_ring) == 16 && offsetof(fmd_meter_status, peak_call) == 256 &&
              offsetof(fmd_meter_status, peak_hold) == 264 && offsetof(fmd_meter_status, below_gate) == 272, "fmd_meter_status layout");

struct MeterCoef {
    double pb0, pb1, pb2, npa1, npa2;    // pre-filter b, -a1, -a2
    double rb0, rb1, rb2, nra1, nra2;    // RLB b, -a1, -a2
    double nsb;                          // (double)Nsb
    int Nsb;
};

// in [C][in_stride][2]; status [C]; carry [C][2][5]; hist [C][1000]; edge [1001]
__global__ __launch_bounds__(kT) void k_meter(const float* __restrict__ in, long long in_stride, long long n, const uint8_t* __restrict__ active, int C,
                                              MeterCoef k, const double* __restrict__ edge, fmd_meter_status* __restrict__ status,
                                              double* __restrict__ carry, unsigned* __restrict__ hist) {
    __shared__ __attribute__((aligned(16))) float xs[kT * kRow];
    const int lane = threadIdx.x, rail = lane & 1;
    const int c0 = blockIdx.x * kCh, c = c0 + (lane >> 1);
    const bool live = c < C && (!active || active[c] != 0);
    // which of the workgroup's stations are metered: bit s for station c0 + s (wave-uniform)
    const int cs = c0 + (lane & (kCh - 1));
    const unsigned long long bal = __ballot(cs < C && (!active || active[cs] != 0));
    const unsigned on = (unsigned)(bal & 0xffffffffull);
    if (on == 0) return;

    double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, acc = 0.0;
    float peak_call = 0.0f, peak_hold = 0.0f;
    unsigned long long G = 0, frames = 0;
    unsigned below = 0, nonfin = 0;
    double e1 = 0.0, e2 = 0.0, e3 = 0.0;     // E_{G-1}, E_{G-2}, E_{G-3} (the owner's)
    int ri = 0;                              // G % 30
    int rem = 0x7fffffff;                    // frames to the end of the open sub-block
    fmd_meter_status* st = status + (live ? c : 0);
    if (live) {
        const double* cr = carry + ((size_t)c * 2 + rail) * kCarry;
        s1 = cr[0]; s2 = cr[1]; t1 = cr[2]; t2 = cr[3]; acc = cr[4];
        peak_hold = st->peak_hold[rail];
        frames = st->frames;
        G = st->subblocks;
        rem = k.Nsb - (int)(frames - G * (unsigned long long)k.Nsb);
        if (rail == 0) {
            below = st->below_gate;
            nonfin = st->nonfinite;
            ri = (int)(G % kMeterRing);
            e1 = st->energy_ring[(ri + kMeterRing - 1) % kMeterRing];
            e2 = st->energy_ring[(ri + kMeterRing - 2) % kMeterRing];
            e3 = st->energy_ring[(ri + kMeterRing - 3) % kMeterRing];
        }
    }

    float2 pre[kCh];
    auto fetch = [&](long long f0) {
        const long long f = f0 + lane;
#pragma unroll
        for (int s = 0; s < kCh; s++) {
            pre[s] = make_float2(0.0f, 0.0f);
            if (((on >> s) & 1u) && f < n)                                   // (the first test is wave-uniform)
                pre[s] = *reinterpret_cast<const float2*>(in + ((size_t)(c0 + s) * (size_t)in_stride + (size_t)f) * 2);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int s = 0; s < kCh; s++) {
            xs[(2 * s) * kRow + lane] = pre[s].x;
            xs[(2 * s + 1) * kRow + lane] = pre[s].y;
        }
    };
    auto step = [&](float x) {
        const double v = (double)x;
        const double o1 = fma(k.pb0, v, s1);
        s1 = fma(k.npa1, o1, fma(k.pb1, v, s2));
        s2 = fma(k.npa2, o1, k.pb2 * v);
        const double o2 = fma(k.rb0, o1, t1);
        t1 = fma(k.nra1, o2, fma(k.rb1, o1, t2));
        t2 = fma(k.nra2, o2, k.rb2 * o1);
        acc = fma(o2, o2, acc);
        peak_call = fmaxf(peak_call, fabsf(x));
        if (--rem == 0) {                                                    // both lanes of a station get here together
            const double other = __shfl_xor(acc, 1);
            if (rail == 0) {
                const double E = (acc + other) / k.nsb;
                st->energy_ring[ri] = E;
                if (G >= 3) {
                    const double B = (((e3 + e2) + e1) + E) * 0.25;
                    if (!(fabs(B) <= 1.7976931348623157e308)) nonfin++;      // inf or NaN
                    else if (B < edge[0]) below++;
                    else {
                        int lo = 0, hi = kMeterBins;                         // edge[lo] <= B; B < edge[hi] or hi == 1000
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            if (edge[mid] <= B) lo = mid; else hi = mid;
                        }
                        hist[(size_t)c * kMeterBins + lo]++;
                    }
                }
                e3 = e2; e2 = e1; e1 = E;
                ri = ri + 1 == kMeterRing ? 0 : ri + 1;
            }
            G++;
            acc = 0.0;
            rem = k.Nsb;
        }
    };

    fetch(0);
    for (long long f0 = 0; f0 < n; f0 += kTile) {
        stash();
        __syncthreads();
        fetch(f0 + kTile);                                                   // in flight while this tile runs (nothing is loaded past n)
        const int cnt = n - f0 < kTile ? (int)(n - f0) : kTile;
        const float* row = &xs[lane * kRow];
        for (int f = 0; f < cnt; f += 4) {
            const float4 q = *reinterpret_cast<const float4*>(row + f);
            step(q.x);
            if (f + 1 < cnt) step(q.y);
            if (f + 2 < cnt) step(q.z);
            if (f + 3 < cnt) step(q.w);
        }
        __syncthreads();
    }

    if (!live) return;
    double* cw = carry + ((size_t)c * 2 + rail) * kCarry;
    cw[0] = s1; cw[1] = s2; cw[2] = t1; cw[3] = t2; cw[4] = acc;
    st->peak_call[rail] = peak_call;
    st->peak_hold[rail] = fmaxf(peak_hold, peak_call);      // (no peak is ever a NaN, so the maximum may be taken in any order)
    if (rail == 0) {
        st->frames = frames + (unsigned long long)n;
        st->subblocks = G;
        st->below_gate = below;
        st->nonfinite = nonfin;
    }
}

}  // namespace

struct fmd_meter_s {
    int device = 0, C = 0, fs = 0;
    long long max_in = 0;
    fmd_meter_design_t design{};
    MeterCoef coef{};
    fmd_meter_status* d_status = nullptr;   // [C]
    double* d_carry = nullptr;              // [C][2][5]
    unsigned* d_hist = nullptr;             // [C][1000]
    double* d_edge = nullptr;               // [1001]
    hipEvent_t done = nullptr;              // end of the previous call's work
    bool have_done = false;
    std::string err;
};

static int mt_fail(fmd_meter m, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    if (m) m->err = buf; else fmd::meter_global_error() = buf;
    return code;
}

static bool mt_quiesce(fmd_meter m) {
    return hipSetDevice(m->device) == hipSuccess && (!m->have_done || hipEventSynchronize(m->done) == hipSuccess);
}

extern "C" {

int fmd_meter_create(const fmd_meter_config* cfg, fmd_meter* out) {
    if (!cfg || !out) return mt_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->n_channels <= 0 || cfg->max_input_frames <= 0 || cfg->max_input_frames > (1LL << 30))
        return mt_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_frames %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_frames);
    fmd_meter_design_t d;
    if (fmd::meter_design(cfg->fs, &d, &fmd::meter_global_error()) != FMD_OK) return FMD_ERR_ARG;
    if (fmd_device_count() <= 0) return mt_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return mt_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_meter m = new fmd_meter_s();
    m->device = dev; m->C = cfg->n_channels; m->fs = cfg->fs; m->max_in = cfg->max_input_frames;
    m->design = d;
    m->coef = MeterCoef{d.pre_b[0], d.pre_b[1], d.pre_b[2], -d.pre_a[1], -d.pre_a[2], d.rlb_b[0], d.rlb_b[1], d.rlb_b[2], -d.rlb_a[1], -d.rlb_a[2],
                        (double)d.frames_per_subblock, d.frames_per_subblock};
    const size_t C = (size_t)m->C;
    bool ok = hipSetDevice(dev) == hipSuccess;
    ok = ok && hipMalloc(&m->d_status, sizeof(fmd_meter_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_carry, sizeof(double) * 2 * kCarry * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_hist, sizeof(unsigned) * kMeterBins * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_edge, sizeof(double) * (kMeterBins + 1)) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&m->done, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMemcpy(m->d_edge, d.edge, sizeof(double) * (kMeterBins + 1), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok || fmd_meter_reset(m, -1) != FMD_OK) { fmd_meter_destroy(m); return mt_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed"); }
    *out = m;
    return FMD_OK;
}

int fmd_meter_destroy(fmd_meter m) {
    if (!m) return FMD_ERR_ARG;
    (void)mt_quiesce(m);
    for (void* p : {(void*)m->d_status, (void*)m->d_carry, (void*)m->d_hist, (void*)m->d_edge})
        if (p) (void)hipFree(p);
    if (m->done) (void)hipEventDestroy(m->done);
    delete m;
    return FMD_OK;
}

int fmd_meter_reset(fmd_meter m, int channel) {
    if (!m) return FMD_ERR_ARG;
    if (channel < -1 || channel >= m->C) return mt_fail(m, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, m->C);
    if (!mt_quiesce(m)) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    const size_t c0 = channel < 0 ? 0 : (size_t)channel, cn = channel < 0 ? (size_t)m->C : 1;
    if (hipMemset(m->d_status + c0, 0, sizeof(fmd_meter_status) * cn) != hipSuccess ||
        hipMemset(m->d_carry + c0 * 2 * kCarry, 0, sizeof(double) * 2 * kCarry * cn) != hipSuccess ||
        hipMemset(m->d_hist + c0 * kMeterBins, 0, sizeof(unsigned) * kMeterBins * cn) != hipSuccess)
        return mt_fail(m, FMD_ERR_DEVICE, "memset failed");
    if (hipStreamSynchronize(nullptr) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");   // done before a later call on any stream
    return FMD_OK;
}

int fmd_meter_reset_peaks(fmd_meter m, int channel) {
    if (!m) return FMD_ERR_ARG;
    if (channel < -1 || channel >= m->C) return mt_fail(m, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, m->C);
    if (!mt_quiesce(m)) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    const size_t c0 = channel < 0 ? 0 : (size_t)channel, cn = channel < 0 ? (size_t)m->C : 1;
    char* p = reinterpret_cast<char*>(m->d_status + c0) + offsetof(fmd_meter_status, peak_call);
    if (hipMemset2D(p, sizeof(fmd_meter_status), 0, 4 * sizeof(float), cn) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "memset failed");
    if (hipStreamSynchronize(nullptr) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    return FMD_OK;
}

int fmd_meter_process_f32_dev(fmd_meter m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, void* stream) {
    if (!m) return FMD_ERR_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return mt_fail(m, FMD_ERR_ARG, "null input, or input not aligned to 8 bytes");
    if (n < 0 || n > in_stride || n > m->max_in)
        return mt_fail(m, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or above max_input_frames %lld", n, in_stride, m->max_in);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipSetDevice(m->device) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "hipSetDevice failed");
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (m->have_done && hipStreamWaitEvent(s, m->done, 0) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "stream wait failed");
    hipLaunchKernelGGL(k_meter, dim3((unsigned)((m->C + kCh - 1) / kCh)), dim3(kT), 0, s, d_in, in_stride, n, d_active, m->C, m->coef, m->d_edge,
                       m->d_status, m->d_carry, m->d_hist);
    if (hipGetLastError() != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "k_meter launch failed");
    if (hipEventRecord(m->done, s) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "event record failed");
    m->have_done = true;
    return FMD_OK;
}

int fmd_meter_get_status(fmd_meter m, fmd_meter_status* out) {
    if (!m || !out) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    if (!mt_quiesce(m)) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, m->d_status, sizeof(fmd_meter_status) * (size_t)m->C, hipMemcpyDeviceToHost) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_meter_get_histogram(fmd_meter m, unsigned* hist) {
    if (!m || !hist) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    if (!mt_quiesce(m)) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(hist, m->d_hist, sizeof(unsigned) * kMeterBins * (size_t)m->C, hipMemcpyDeviceToHost) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_meter_status_dev(fmd_meter m, const fmd_meter_status** d_status) {
    if (!m || !d_status) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    *d_status = m->d_status;
    return FMD_OK;
}

const char* fmd_meter_last_error(fmd_meter m) { return m ? m->err.c_str() : fmd::meter_global_error().c_str(); }

}  // extern "C"
