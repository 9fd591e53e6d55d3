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
// With FMD_METER_RANGE the call runs k_meter<true>, which at each sub-block end from the 30th on also classifies the short-term window (the
// ring's 30 energies) into a second histogram; k_meter<false> is the kernel as it was.  With FMD_METER_TRUE_PEAK a second kernel, k_meter_tp,
// follows on the same stream: a 4x (or 2x) polyphase interpolator over every sample, parallel in time (below).
//
// Denormals: fp64 and fp32 denormals are kept (hipcc's default mode; this file is NOT built with -fgpu-flush-denormals-to-zero).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "fmd_meter_design.h"
#include "fmd_side.h"
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

// in [C][in_stride][2]; status [C]; carry [C][2][5]; hist [C][1000]; edge [1001]; with kRange r128 [C] and range_hist [C][1000]
template <bool kRange>
__global__ __launch_bounds__(kT) void k_meter(const float* __restrict__ in, long long in_stride, long long n, const uint8_t* __restrict__ active, int C,
                                              MeterCoef k, const double* __restrict__ edge, fmd_meter_status* __restrict__ status,
                                              double* __restrict__ carry, unsigned* __restrict__ hist, fmd_meter_r128_status* __restrict__ r128,
                                              unsigned* __restrict__ range_hist) {
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
    unsigned st_below = 0, st_nonfin = 0;    // (kRange: the short-term values' counters)
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
            if (kRange) { st_below = r128[c].st_below; st_nonfin = r128[c].st_nonfinite; }
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
                if (kRange && G >= (unsigned long long)(kMeterRing - 1)) {    // the short-term window: sub-blocks G - 29 ... G, oldest first
                    double sum = 0.0;
                    int i = ri + 1 == kMeterRing ? 0 : ri + 1;
                    for (int j = 0; j < kMeterRing; j++) {
                        sum += st->energy_ring[i];
                        i = i + 1 == kMeterRing ? 0 : i + 1;
                    }
                    const double S = sum / 30.0;
                    if (!(fabs(S) <= 1.7976931348623157e308)) st_nonfin++;
                    else if (S < edge[0]) st_below++;
                    else {
                        int lo = 0, hi = kMeterBins;
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            if (edge[mid] <= S) lo = mid; else hi = mid;
                        }
                        range_hist[(size_t)c * kMeterBins + lo]++;
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
        if (kRange) { r128[c].st_below = st_below; r128[c].st_nonfinite = st_nonfin; }
    }
}

// ---- true peak ------------------------------------------------------------------------------------------------------------------------
//
// No recurrence in time: one workgroup of 256 threads per station walks the station's frames in tiles of 1024.  A tile and the 11 frames
// before it (the station's history for the first tile, the input itself after it) are loaded coalesced, 16 bytes a lane where the station's
// row is 16-byte aligned and 8 otherwise, and de-interleaved into one LDS row per rail; the row starts 12 floats before the tile, so the
// thread that owns frames 4t ... 4t + 3 reads its 16-float window (x[4t - 12] ... x[4t + 3]) as four aligned 16-byte reads per rail,
// consecutive lanes 16 bytes apart.  Per frame and rail the three phases are three independent chains of twelve fmas; the 36 taps are a
// kernel argument and sit in SGPRs.  The maximum is folded per thread, across the wavefront by cross-lane moves, across the four wavefronts
// through LDS; thread 0 alone stores the station's four floats, and threads 0 ... 21 the new history.  No atomics.
constexpr int kTpT = 256;                        // threads per workgroup
constexpr int kTpTile = 4 * kTpT;                // frames per tile
constexpr int kTpLead = 12;                      // floats of an LDS row before the tile's first frame (11 of history behind one unused)
constexpr int kTpRow = kTpLead + kTpTile;        // floats per LDS row
constexpr int kTpH = fmd::kMeterTpHist;          // 11
static_assert(kTpH == 11 && kTpLead == kTpH + 1 && 2 * kTpH <= kTpT, "k_meter_tp's window");
static_assert(sizeof(fmd_meter_r128_status) == 24 && offsetof(fmd_meter_r128_status, tp_hold) == 8 && offsetof(fmd_meter_r128_status, st_below) == 16,
              "fmd_meter_r128_status layout");

struct TpTaps { float g[3][12]; };

// in [C][in_stride][2]; r128 [C]; tphist [C][2][11]
template <int L>
__global__ __launch_bounds__(kTpT) void k_meter_tp(const float* __restrict__ in, long long in_stride, long long n, const uint8_t* __restrict__ active,
                                                   TpTaps taps, fmd_meter_r128_status* __restrict__ r128, float* __restrict__ tphist) {
    __shared__ __attribute__((aligned(16))) float xs[2 * kTpRow];
    __shared__ float red[2 * (kTpT / 64)];
    const int c = blockIdx.x, t = threadIdx.x;
    if (active && active[c] == 0) return;                                    // (uniform over the workgroup)
    const float* base = in + (size_t)c * (size_t)in_stride * 2;
    float* hs = tphist + (size_t)c * 2 * kTpH;
    const bool wide = (reinterpret_cast<uintptr_t>(base) & 15) == 0;         // 16-byte loads: every tile starts a multiple of 8 KB in

    // the history this call leaves: frame n - 11 + k for slot k, taken from the input, or from the old history where the call is shorter.
    // Every read of the old history happens before the first barrier, every write after the last.
    float hnew = 0.0f;
    if (t < 2 * kTpH) {
        const int r = t / kTpH, kk = t - r * kTpH;
        const long long i = n - kTpH + kk;
        hnew = i >= 0 ? base[(size_t)i * 2 + r] : hs[r * kTpH + (int)(n + kk)];
    }

    float4 pre[2];                                                           // two frames each; wide: 2 loads of 16 bytes, else 4 of 8
    float halo = 0.0f;
    auto fetch = [&](long long f0) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const long long f = f0 + q * (2 * kTpT) + 2 * t;
            pre[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (f + 1 < n) {
                if (wide) pre[q] = *reinterpret_cast<const float4*>(base + (size_t)f * 2);
                else {
                    const float2 a = *reinterpret_cast<const float2*>(base + (size_t)f * 2);
                    const float2 b = *reinterpret_cast<const float2*>(base + (size_t)f * 2 + 2);
                    pre[q] = make_float4(a.x, a.y, b.x, b.y);
                }
            } else if (f < n) {
                const float2 a = *reinterpret_cast<const float2*>(base + (size_t)f * 2);
                pre[q] = make_float4(a.x, a.y, 0.0f, 0.0f);
            }
        }
        if (L > 1 && t < 2 * kTpH && f0 < n) {                               // the 11 frames before the tile, per rail
            const int r = t / kTpH, kk = t - r * kTpH;
            halo = f0 == 0 ? hs[r * kTpH + kk] : base[(size_t)(f0 - kTpH + kk) * 2 + r];
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int o = kTpLead + q * (2 * kTpT) + 2 * t;
            *reinterpret_cast<float2*>(&xs[o]) = make_float2(pre[q].x, pre[q].z);
            *reinterpret_cast<float2*>(&xs[kTpRow + o]) = make_float2(pre[q].y, pre[q].w);
        }
        if (L > 1 && t < 2 * kTpH) {
            const int r = t / kTpH, kk = t - r * kTpH;
            xs[r * kTpRow + 1 + kk] = halo;
        }
    };

    float tp[2] = {0.0f, 0.0f};
    fetch(0);
    for (long long f0 = 0; f0 < n; f0 += kTpTile) {
        stash();
        __syncthreads();
        fetch(f0 + kTpTile);                                                 // in flight while this tile runs (nothing is loaded past n)
        const int cnt = n - f0 < kTpTile ? (int)(n - f0) : kTpTile;
        if (4 * t < cnt) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const float* row = &xs[r * kTpRow + 4 * t];
                float w[16];                                                 // w[i] = x[4t - 12 + i]
                if (L > 1) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const float4 v = *reinterpret_cast<const float4*>(row + 4 * q);
                        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
                    }
                } else {
                    const float4 v = *reinterpret_cast<const float4*>(row + kTpLead);
                    w[12] = v.x; w[13] = v.y; w[14] = v.z; w[15] = v.w;
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    float m = fabsf(w[12 + j]);
#pragma unroll
                    for (int p = 0; p < L - 1; p++) {
                        float y = 0.0f;
#pragma unroll
                        for (int kk = 0; kk < 12; kk++) y = fmaf(taps.g[p][kk], w[12 + j - kk], y);
                        m = fmaxf(m, fabsf(y));                              // (a NaN is dropped: fmaxf returns its other operand)
                    }
                    if (4 * t + j < cnt) tp[r] = fmaxf(tp[r], m);
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < 2; r++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) tp[r] = fmaxf(tp[r], __shfl_xor(tp[r], d));
        if ((t & 63) == 0) red[r * (kTpT / 64) + (t >> 6)] = tp[r];
    }
    __syncthreads();
    if (t < 2 * kTpH) hs[t] = hnew;
    if (t == 0) {
        fmd_meter_r128_status* st = r128 + c;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            float m = red[r * (kTpT / 64)];
#pragma unroll
            for (int wv = 1; wv < kTpT / 64; wv++) m = fmaxf(m, red[r * (kTpT / 64) + wv]);
            st->tp_call[r] = m;
            st->tp_hold[r] = fmaxf(st->tp_hold[r], m);
        }
    }
}

}  // namespace

struct fmd_meter_s {
    int C = 0, fs = 0;
    long long max_in = 0;
    fmd_meter_design_t design{};
    MeterCoef coef{};
    fmd_meter_status* d_status = nullptr;   // [C]
    double* d_carry = nullptr;              // [C][2][5]
    unsigned* d_hist = nullptr;             // [C][1000]
    double* d_edge = nullptr;               // [1001]
    unsigned features = 0;                  // FMD_METER_*
    fmd_meter_tp_design_t tp{};
    TpTaps tp_taps{};
    fmd_meter_r128_status* d_r128 = nullptr;   // [C], with either feature
    float* d_tphist = nullptr;              // [C][2][11], with FMD_METER_TRUE_PEAK
    unsigned* d_range = nullptr;            // [C][1000], with FMD_METER_RANGE
    fmd::CallOrder order;                   // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int mt_fail(fmd_meter m, int code, const char* fmt, A... args) { return fmd::fail(m ? m->err : fmd::meter_global_error(), code, fmt, args...); }

extern "C" {

int fmd_meter_create(const fmd_meter_config* cfg, fmd_meter* out) { return fmd_meter_create_ex(cfg, 0u, out); }

int fmd_meter_create_ex(const fmd_meter_config* cfg, unsigned features, fmd_meter* out) {
    if (!cfg || !out) return mt_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (features & ~(FMD_METER_TRUE_PEAK | FMD_METER_RANGE)) return mt_fail(nullptr, FMD_ERR_ARG, "unknown feature bits 0x%x", features);
    if (cfg->n_channels <= 0 || cfg->max_input_frames <= 0 || cfg->max_input_frames > (1LL << 30))
        return mt_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_frames %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_frames);
    fmd_meter_design_t d;
    if (fmd::meter_design(cfg->fs, &d, &fmd::meter_global_error()) != FMD_OK) return FMD_ERR_ARG;
    fmd_meter_tp_design_t tp;
    if (fmd::meter_tp_design(cfg->fs, &tp, &fmd::meter_global_error()) != FMD_OK) return FMD_ERR_ARG;
    if (fmd_device_count() <= 0) return mt_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return mt_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_meter m = new fmd_meter_s();
    m->C = cfg->n_channels; m->fs = cfg->fs; m->max_in = cfg->max_input_frames;
    m->design = d;
    m->features = features;
    m->tp = tp;
    for (int p = 0; p < 3; p++)
        for (int kk = 0; kk < fmd::kMeterTpTaps; kk++) m->tp_taps.g[p][kk] = tp.taps[p][kk];
    m->coef = MeterCoef{d.pre_b[0], d.pre_b[1], d.pre_b[2], -d.pre_a[1], -d.pre_a[2], d.rlb_b[0], d.rlb_b[1], d.rlb_b[2], -d.rlb_a[1], -d.rlb_a[2],
                        (double)d.frames_per_subblock, d.frames_per_subblock};
    const size_t C = (size_t)m->C;
    bool ok = m->order.init(dev);
    ok = ok && hipMalloc(&m->d_status, sizeof(fmd_meter_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_carry, sizeof(double) * 2 * kCarry * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_hist, sizeof(unsigned) * kMeterBins * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_edge, sizeof(double) * (kMeterBins + 1)) == hipSuccess;
    if (features) ok = ok && hipMalloc(&m->d_r128, sizeof(fmd_meter_r128_status) * C) == hipSuccess;
    if (features & FMD_METER_TRUE_PEAK) ok = ok && hipMalloc(&m->d_tphist, sizeof(float) * 2 * kTpH * C) == hipSuccess;
    if (features & FMD_METER_RANGE) ok = ok && hipMalloc(&m->d_range, sizeof(unsigned) * kMeterBins * C) == hipSuccess;
    ok = ok && hipMemcpy(m->d_edge, d.edge, sizeof(double) * (kMeterBins + 1), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok || fmd_meter_reset(m, -1) != FMD_OK) { fmd_meter_destroy(m); return mt_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed"); }
    *out = m;
    return FMD_OK;
}

int fmd_meter_destroy(fmd_meter m) {
    if (!m) return FMD_ERR_ARG;
    (void)m->order.quiesce();
    for (void* p : {(void*)m->d_status, (void*)m->d_carry, (void*)m->d_hist, (void*)m->d_edge, (void*)m->d_r128, (void*)m->d_tphist, (void*)m->d_range})
        if (p) (void)hipFree(p);
    delete m;
    return FMD_OK;
}

int fmd_meter_reset(fmd_meter m, int channel) {
    if (!m) return FMD_ERR_ARG;
    int first, count;
    if (!fmd::channel_range(channel, m->C, &first, &count)) return mt_fail(m, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, m->C);
    if (!m->order.quiesce()) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    const size_t c0 = (size_t)first, cn = (size_t)count;
    if (hipMemset(m->d_status + c0, 0, sizeof(fmd_meter_status) * cn) != hipSuccess ||
        hipMemset(m->d_carry + c0 * 2 * kCarry, 0, sizeof(double) * 2 * kCarry * cn) != hipSuccess ||
        hipMemset(m->d_hist + c0 * kMeterBins, 0, sizeof(unsigned) * kMeterBins * cn) != hipSuccess ||
        (m->d_r128 && hipMemset(m->d_r128 + c0, 0, sizeof(fmd_meter_r128_status) * cn) != hipSuccess) ||
        (m->d_tphist && hipMemset(m->d_tphist + c0 * 2 * kTpH, 0, sizeof(float) * 2 * kTpH * cn) != hipSuccess) ||
        (m->d_range && hipMemset(m->d_range + c0 * kMeterBins, 0, sizeof(unsigned) * kMeterBins * cn) != hipSuccess))
        return mt_fail(m, FMD_ERR_DEVICE, "memset failed");
    if (hipStreamSynchronize(nullptr) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");   // done before a later call on any stream
    return FMD_OK;
}

int fmd_meter_reset_peaks(fmd_meter m, int channel) {
    if (!m) return FMD_ERR_ARG;
    int first, count;
    if (!fmd::channel_range(channel, m->C, &first, &count)) return mt_fail(m, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, m->C);
    if (!m->order.quiesce()) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    const size_t c0 = (size_t)first, cn = (size_t)count;
    char* p = reinterpret_cast<char*>(m->d_status + c0) + offsetof(fmd_meter_status, peak_call);
    if (hipMemset2D(p, sizeof(fmd_meter_status), 0, 4 * sizeof(float), cn) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "memset failed");
    // tp_call and tp_hold, the record's first 16 bytes (the interpolator's history stays)
    if (m->d_r128 && hipMemset2D(m->d_r128 + c0, sizeof(fmd_meter_r128_status), 0, 4 * sizeof(float), cn) != hipSuccess)
        return mt_fail(m, FMD_ERR_DEVICE, "memset failed");
    if (hipStreamSynchronize(nullptr) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    return FMD_OK;
}

int fmd_meter_process_f32_dev(fmd_meter m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, void* stream) {
    if (!m) return FMD_ERR_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return mt_fail(m, FMD_ERR_ARG, "null input, or input not aligned to 8 bytes");
    if (n < 0 || n > in_stride || n > m->max_in)
        return mt_fail(m, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or above max_input_frames %lld", n, in_stride, m->max_in);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* e = m->order.begin(s)) return mt_fail(m, FMD_ERR_DEVICE, "%s", e);
    const dim3 grid((unsigned)((m->C + kCh - 1) / kCh));
    if (m->features & FMD_METER_RANGE)
        hipLaunchKernelGGL(k_meter<true>, grid, dim3(kT), 0, s, d_in, in_stride, n, d_active, m->C, m->coef, m->d_edge, m->d_status, m->d_carry,
                           m->d_hist, m->d_r128, m->d_range);
    else
        hipLaunchKernelGGL(k_meter<false>, grid, dim3(kT), 0, s, d_in, in_stride, n, d_active, m->C, m->coef, m->d_edge, m->d_status, m->d_carry,
                           m->d_hist, static_cast<fmd_meter_r128_status*>(nullptr), static_cast<unsigned*>(nullptr));
    if (hipGetLastError() != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "k_meter launch failed");
    if (m->features & FMD_METER_TRUE_PEAK) {                                 // one workgroup per station, behind k_meter
        const dim3 tgrid((unsigned)m->C);
        if (m->tp.L == 4) hipLaunchKernelGGL(k_meter_tp<4>, tgrid, dim3(kTpT), 0, s, d_in, in_stride, n, d_active, m->tp_taps, m->d_r128, m->d_tphist);
        else if (m->tp.L == 2) hipLaunchKernelGGL(k_meter_tp<2>, tgrid, dim3(kTpT), 0, s, d_in, in_stride, n, d_active, m->tp_taps, m->d_r128, m->d_tphist);
        else hipLaunchKernelGGL(k_meter_tp<1>, tgrid, dim3(kTpT), 0, s, d_in, in_stride, n, d_active, m->tp_taps, m->d_r128, m->d_tphist);
        if (hipGetLastError() != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "k_meter_tp launch failed");
    }
    if (const char* e = m->order.end(s)) return mt_fail(m, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_meter_get_status(fmd_meter m, fmd_meter_status* out) {
    if (!m || !out) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    if (!m->order.quiesce()) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, m->d_status, sizeof(fmd_meter_status) * (size_t)m->C, hipMemcpyDeviceToHost) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_meter_get_histogram(fmd_meter m, unsigned* hist) {
    if (!m || !hist) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    if (!m->order.quiesce()) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(hist, m->d_hist, sizeof(unsigned) * kMeterBins * (size_t)m->C, hipMemcpyDeviceToHost) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_meter_status_dev(fmd_meter m, const fmd_meter_status** d_status) {
    if (!m || !d_status) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    *d_status = m->d_status;
    return FMD_OK;
}

int fmd_meter_features(fmd_meter m, unsigned* features) {
    if (!m || !features) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    *features = m->features;
    return FMD_OK;
}

int fmd_meter_get_r128_status(fmd_meter m, fmd_meter_r128_status* out) {
    if (!m || !out) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    if (!m->features) return mt_fail(m, FMD_ERR_STATE, "the meter was created without FMD_METER_TRUE_PEAK or FMD_METER_RANGE");
    if (!m->order.quiesce()) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, m->d_r128, sizeof(fmd_meter_r128_status) * (size_t)m->C, hipMemcpyDeviceToHost) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_meter_r128_status_dev(fmd_meter m, const fmd_meter_r128_status** d_out) {
    if (!m || !d_out) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    if (!m->features) return mt_fail(m, FMD_ERR_STATE, "the meter was created without FMD_METER_TRUE_PEAK or FMD_METER_RANGE");
    *d_out = m->d_r128;
    return FMD_OK;
}

int fmd_meter_get_range_histogram(fmd_meter m, unsigned* hist) {
    if (!m || !hist) return mt_fail(m, FMD_ERR_ARG, "null meter or output");
    if (!(m->features & FMD_METER_RANGE)) return mt_fail(m, FMD_ERR_STATE, "the meter was created without FMD_METER_RANGE");
    if (!m->order.quiesce()) return mt_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(hist, m->d_range, sizeof(unsigned) * kMeterBins * (size_t)m->C, hipMemcpyDeviceToHost) != hipSuccess) return mt_fail(m, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

const char* fmd_meter_last_error(fmd_meter m) { return m ? m->err.c_str() : fmd::meter_global_error().c_str(); }

}  // extern "C"
