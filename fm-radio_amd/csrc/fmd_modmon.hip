// FM modulation monitor, device side (include/fmdemod.h, "FM modulation monitor").
//
// NOT in the reference.  Peak deviation per 50 ms interval and its histogram, the multiplex power's sums per second, the carrier offset
// and the pilot's correlation sums of every station, read in place from the station baseband [C][in_stride][2] (cf32 or u8) that the
// demodulator takes and the channeliser writes.
//
// One kernel per call, k_modmon<format>: theta, d and y of a sample depend only on the 33 samples behind it, so the work is parallel in
// time and only the order inside a partial sum binds.  One wavefront per station; the lane is r mod 64, r the sample's place in its 50 ms
// interval, so lane j owns partial j of the four interval sums outright and adds its terms in ascending r.  The wavefront walks rows of 64
// consecutive samples (one coalesced 512-byte load for cf32, 128 bytes for u8, non-temporal: the IQ is read once), four rows in registers
// ahead of the row it works on.  A row starts at a multiple of 64 of r, so the first row of a call and the rows around an interval's end
// are partial (lanes masked); an interval's end is wave-uniform.  Neighbouring samples meet through two wavefront-private LDS rings
// indexed by the sample's place in the call: theta (one read of the lane before) and d (written twice, 128 floats apart, so that the 33
// reads of a lane are one descending run of addresses that the compiler pairs into ds_read2_b32).  The taps, hz_per_rad and the counters
// are kernel arguments or wave-uniform values (SGPRs); the pilot table sits in LDS.  At an interval's end the partials fold by
// cross-lane moves in the contract's halving order and lane 0 alone classifies and stores, with ordinary stores.  No atomics, no scratch.
//
// Denormals: fp64 and fp32 denormals are kept (hipcc's default mode; this file is NOT built with -fgpu-flush-denormals-to-zero).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "fmd_iq.h"
#include "fmd_math.h"
#include "fmd_modmon_design.h"
#include "fmd_rows.h"
#include "fmd_side.h"
#include "fmdemod.h"

using fmd::kModmonBins;
using fmd::kModmonHist;
using fmd::kModmonMaxP;
using fmd::kModmonPartials;
using fmd::kModmonRing;
using fmd::kModmonTaps;

namespace {

constexpr int kT = 64;               // threads per workgroup: one wavefront, one station
constexpr int kPf = 4;               // rows loaded ahead
constexpr int kSlots = 128;          // slots of the LDS rings (a row and the 33 samples behind it fit twice over)
constexpr int kCarryF = 4 + kModmonHist;   // floats per station: hi, lo of the open interval, theta[n - 1], unused, d[n - 32 ... n - 1]
constexpr int kCarryD = 4 * kModmonPartials;   // doubles per station: the open interval's s1, s2, sc, ss partials
static_assert(kModmonPartials == kT && kModmonTaps == 33 && kModmonHist + kT <= kSlots, "k_modmon's lane and ring layout");

static_assert(sizeof(fmd_modmon_status) == 1792 && offsetof(fmd_modmon_status, intervals) == 8 && offsetof(fmd_modmon_status, seconds) == 16 &&
              offsetof(fmd_modmon_status, last_hi) == 24 && offsetof(fmd_modmon_status, last_lo) == 28 && offsetof(fmd_modmon_status, hold_hi) == 32 &&
              offsetof(fmd_modmon_status, hold_lo) == 36 && offsetof(fmd_modmon_status, last_s1) == 40 && offsetof(fmd_modmon_status, last_s2) == 48 &&
              offsetof(fmd_modmon_status, last_sc) == 56 && offsetof(fmd_modmon_status, last_ss) == 64 && offsetof(fmd_modmon_status, sec_e) == 72 &&
              offsetof(fmd_modmon_status, sec_f) == 552 && offsetof(fmd_modmon_status, sec_q) == 1032 && offsetof(fmd_modmon_status, sec_n) == 1512 &&
              offsetof(fmd_modmon_status, open_e) == 1752 && offsetof(fmd_modmon_status, open_f) == 1760 && offsetof(fmd_modmon_status, open_q) == 1768 &&
              offsetof(fmd_modmon_status, open_n) == 1776 && offsetof(fmd_modmon_status, over) == 1780 && offsetof(fmd_modmon_status, nonfinite) == 1784 &&
              offsetof(fmd_modmon_status, reserved) == 1788, "fmd_modmon_status layout");
static_assert(kModmonRing == 60 && kModmonBins == 300 && sizeof(((fmd_modmon_design_t*)nullptr)->pilot_cos) == sizeof(double) * kModmonMaxP, "fmd_modmon layout constants");

struct MmTaps { float h[kModmonTaps]; };

typedef float mm_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 mm_load(const float2* p) {
    const mm_f2 v = __builtin_nontemporal_load(reinterpret_cast<const mm_f2*>(p));
    return make_float2(v.x, v.y);
}
__device__ __forceinline__ unsigned short mm_load(const unsigned short* p) { return __builtin_nontemporal_load(p); }

__device__ __forceinline__ float mm_wrap(float x) {
    const float pi = fmd::bits_f32(fmd::kPiBits);
    if (x >= pi) return x - 2.0f * pi;
    if (x <= -pi) return x + 2.0f * pi;
    return x;
}

constexpr float kInf = __builtin_inff();

// Orders the wavefront's LDS writes before its later LDS reads.  The workgroup is one wavefront, whose LDS instructions execute in issue
// order, so nothing has to be waited for: the fences and the barrier only keep the compiler from moving memory operations across this
// point.  (__syncthreads() would also wait for the global loads in flight, the rows fetched ahead.)
__device__ __forceinline__ void mm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// in [C][in_stride] IQ pairs; pilot [2][384]; status [C]; part [C][4][64]; carry [C][36]; hist [C][300]
template <typename S>
__global__ __launch_bounds__(kT) void k_modmon(const typename fmd::Iq<S>::raw* __restrict__ in, long long in_stride, long long n,
                                               const uint8_t* __restrict__ active, MmTaps taps, double hz_per_rad, int M, int P,
                                               const double* __restrict__ pilot, fmd_modmon_status* __restrict__ status, double* __restrict__ part,
                                               float* __restrict__ carry, unsigned* __restrict__ hist) {
    using raw = typename fmd::Iq<S>::raw;
    __shared__ double pc[kModmonMaxP], ps[kModmonMaxP];
    __shared__ float th_ring[kSlots];
    __shared__ float d_ring[2 * kSlots];
    const int c = blockIdx.x, lane = threadIdx.x;
    if (active && active[c] == 0) return;                                    // (uniform over the wavefront)
    fmd_modmon_status* st = status + c;
    const raw* base = in + (size_t)c * (size_t)in_stride;
    double* pp = part + (size_t)c * kCarryD;
    float* cf = carry + (size_t)c * kCarryF;

    for (int k = lane; k < P; k += kT) { pc[k] = pilot[k]; ps[k] = pilot[kModmonMaxP + k]; }
    // the station's history, at the ring slots of the call's samples -32 ... -1
    if (lane < kModmonHist) {
        const float v = cf[4 + lane];
        d_ring[kSlots - kModmonHist + lane] = v;
        d_ring[2 * kSlots - kModmonHist + lane] = v;
    }
    if (lane == 0) th_ring[kSlots - 1] = cf[2];
    const unsigned long long samples0 = st->samples;
    unsigned long long G = st->intervals;
    int r0 = __builtin_amdgcn_readfirstlane((int)(samples0 - G * (unsigned long long)M));   // the first sample's place in its interval
    const int pm0 = __builtin_amdgcn_readfirstlane((int)(samples0 % (unsigned long long)P));
    const int pstep = kT % P;
    const bool fresh = samples0 == 0;                                        // the call's sample 0 is the station's sample 0: d = +0
    float chi = cf[0], clo = cf[1];                                          // the open interval's extremes before this call
    double s1 = pp[lane], s2 = pp[kT + lane], sc = pp[2 * kT + lane], ss = pp[3 * kT + lane];
    float hi = -kInf, lo = kInf;                                             // the lane's, over the open interval's samples of this call
    float hmax = -kInf, hmin = kInf;                                         // the lane's, over the call
    __syncthreads();

    long long s0 = 0;                                                        // the segment's first sample: a segment ends with its interval or the call
    while (s0 < n) {
        const long long left = (long long)(M - r0);
        const long long seg_end = n - s0 < left ? n : s0 + left;
        const long long rb = s0 - (long long)(r0 & (kT - 1));                // the first row's lane 0 (before s0: those lanes are masked)
        int idx = (int)((unsigned)(pm0 + (int)rb + lane + kT * P) % (unsigned)P);        // (n mod P) of the lane's sample in the row at hand

        raw nxt[kPf];
        auto fetch = [&](long long row) {
#pragma unroll
            for (int p = 0; p < kPf; p++) {
                const long long i = row + (long long)p * kT + lane;
                nxt[p] = fmd::Iq<S>::zero();
                if (i >= 0 && i < n) nxt[p] = mm_load(base + i);
            }
        };
        auto process = [&](raw v, long long row) {
            const long long i = row + lane;
            const bool valid = i >= s0 && i < seg_end;
            const int slot = (int)(i & (kSlots - 1));
            const float2 z = fmd::Iq<S>::cf32(v);
            const float th = fmd::fmd_atan2f(z.y, z.x);
            if (valid) th_ring[slot] = th;
            mm_wave_sync();
            float dd = mm_wrap(th - th_ring[(slot + kSlots - 1) & (kSlots - 1)]);
            if (fresh && i == 0) dd = 0.0f;
            if (valid) { d_ring[slot] = dd; d_ring[slot + kSlots] = dd; }
            mm_wave_sync();
            const float* w = &d_ring[slot + kSlots];                         // w[-t] = d[n - t]
            float y = 0.0f;
#pragma unroll
            for (int t = 0; t < kModmonTaps; t++) y = fmaf(taps.h[t], w[-t], y);
            if (valid) {
                hi = fmaxf(hi, y); lo = fminf(lo, y);
                hmax = fmaxf(hmax, y); hmin = fminf(hmin, y);
                const double fd = (double)y * hz_per_rad;
                s1 = s1 + fd;
                s2 = fma(fd, fd, s2);
                sc = fma(fd, pc[idx], sc);
                ss = fma(fd, ps[idx], ss);
            }
            idx += pstep;
            idx = idx >= P ? idx - P : idx;
        };

        fetch(rb);
        for (long long row = rb; row < seg_end; row += (long long)kPf * kT) {
            raw cur[kPf];
#pragma unroll
            for (int p = 0; p < kPf; p++) cur[p] = nxt[p];
            if (row + (long long)kPf * kT < seg_end) fetch(row + (long long)kPf * kT);   // in flight while these rows run
#pragma unroll
            for (int p = 0; p < kPf; p++)
                if (row + (long long)p * kT < seg_end) process(cur[p], row + (long long)p * kT);
        }

        // the segment's extremes: no operand is ever a NaN, so the order of a maximum does not matter
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { hi = fmaxf(hi, __shfl_xor(hi, d)); lo = fminf(lo, __shfl_xor(lo, d)); }
        chi = fmaxf(chi, hi); clo = fminf(clo, lo);
        hi = -kInf; lo = kInf;
        r0 += (int)(seg_end - s0);
        if (r0 == M) {                                                       // the interval is complete (wave-uniform)
            fmd::rows::fold(s1, s2, sc, ss);
            G++;
            if (lane == 0) {
                const double D = 0.5 * ((double)chi - (double)clo) * hz_per_rad;
                st->last_hi = chi; st->last_lo = clo;
                st->last_s1 = s1; st->last_s2 = s2; st->last_sc = sc; st->last_ss = ss;
                if (!fmd::rows::finite(D) || !fmd::rows::finite(s2)) st->nonfinite++;
                else {
                    if (D >= fmd::kModmonBinHz * (double)kModmonBins) st->over++;
                    else {
                        int bl = 0, bh = kModmonBins;                        // edge[bl] <= D < edge[bh], edge[j] = 500.0 * j exactly
                        while (bh - bl > 1) {
                            const int mid = (bl + bh) >> 1;
                            if (fmd::kModmonBinHz * (double)mid <= D) bl = mid; else bh = mid;
                        }
                        hist[(size_t)c * kModmonBins + bl]++;
                    }
                    st->open_e += s2;
                    st->open_f += s1;
                    st->open_q += fma(sc, sc, ss * ss);
                    st->open_n += 1;
                }
                if (G % fmd::kModmonIntervalsPerSecond == 0) {
                    const unsigned long long sec = st->seconds;
                    const int k = (int)(sec % kModmonRing);
                    st->sec_e[k] = st->open_e; st->sec_f[k] = st->open_f; st->sec_q[k] = st->open_q; st->sec_n[k] = st->open_n;
                    st->seconds = sec + 1;
                    st->open_e = 0.0; st->open_f = 0.0; st->open_q = 0.0; st->open_n = 0;
                }
            }
            s1 = 0.0; s2 = 0.0; sc = 0.0; ss = 0.0;
            chi = -kInf; clo = kInf;
            r0 = 0;
        }
        s0 = seg_end;
    }

    // what the next call needs: the open interval's partials and extremes, and the last 33 samples' theta and d
    pp[lane] = s1; pp[kT + lane] = s2; pp[2 * kT + lane] = sc; pp[3 * kT + lane] = ss;
    float hnew = 0.0f;
    if (lane < kModmonHist) hnew = d_ring[(int)((n - kModmonHist + lane) & (kSlots - 1))];
    const float thnew = th_ring[(int)((n - 1) & (kSlots - 1))];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { hmax = fmaxf(hmax, __shfl_xor(hmax, d)); hmin = fminf(hmin, __shfl_xor(hmin, d)); }
    if (lane < kModmonHist) cf[4 + lane] = hnew;
    if (lane == 0) {
        cf[0] = chi; cf[1] = clo; cf[2] = thnew;
        st->hold_hi = fmaxf(st->hold_hi, hmax);
        st->hold_lo = fminf(st->hold_lo, hmin);
        st->samples = samples0 + (unsigned long long)n;
        st->intervals = G;
    }
}

// a station as after create (everything 0, the extremes at their identities), or with `peaks` its hold_hi and hold_lo alone
__global__ __launch_bounds__(kT) void k_modmon_reset(int c0, int peaks, fmd_modmon_status* __restrict__ status, double* __restrict__ part,
                                                     float* __restrict__ carry, unsigned* __restrict__ hist) {
    const int c = c0 + blockIdx.x, t = threadIdx.x;
    fmd_modmon_status* st = status + c;
    if (!peaks) {
        unsigned* w = reinterpret_cast<unsigned*>(st);
        for (int i = t; i < (int)(sizeof(fmd_modmon_status) / 4); i += kT) w[i] = 0u;
        for (int i = t; i < kCarryD; i += kT) part[(size_t)c * kCarryD + i] = 0.0;
        for (int i = t; i < kCarryF; i += kT) carry[(size_t)c * kCarryF + i] = 0.0f;
        for (int i = t; i < kModmonBins; i += kT) hist[(size_t)c * kModmonBins + i] = 0u;
        __syncthreads();
        if (t == 0) { carry[(size_t)c * kCarryF] = -kInf; carry[(size_t)c * kCarryF + 1] = kInf; }
    }
    if (t == 0) { st->hold_hi = -kInf; st->hold_lo = kInf; }
}

}  // namespace

struct fmd_modmon_s {
    int C = 0, fs = 0;
    long long max_in = 0;
    fmd_modmon_design_t design{};
    MmTaps taps{};
    fmd_modmon_status* d_status = nullptr;  // [C]
    double* d_part = nullptr;               // [C][4][64]
    float* d_carry = nullptr;               // [C][36]
    unsigned* d_hist = nullptr;             // [C][300]
    double* d_pilot = nullptr;              // [2][384]
    fmd::CallOrder order;                   // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int mm_fail(fmd_modmon m, int code, const char* fmt, A... args) { return fmd::fail(m ? m->err : fmd::modmon_global_error(), code, fmt, args...); }

static int mm_reset(fmd_modmon m, int channel, int peaks) {
    if (!m) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, m->C, &c0, &cn)) return mm_fail(m, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, m->C);
    if (!m->order.quiesce()) return mm_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_modmon_reset, dim3((unsigned)cn), dim3(kT), 0, nullptr, c0, peaks, m->d_status, m->d_part, m->d_carry, m->d_hist);
    if (const char* e = fmd::control_end("k_modmon_reset launch failed")) return mm_fail(m, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

template <typename S>
static int mm_process(fmd_modmon m, const void* d_in, size_t align, long long in_stride, long long n, const uint8_t* d_active, void* stream) {
    if (!m) return FMD_ERR_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % align != 0) return mm_fail(m, FMD_ERR_ARG, "null input, or input not aligned to %zu bytes", align);
    if (n < 0 || n > in_stride || n > m->max_in)
        return mm_fail(m, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or above max_input_samples %lld", n, in_stride, m->max_in);
    if (n == 0) return FMD_OK;                                               // nothing of any station changes
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* e = m->order.begin(s)) return mm_fail(m, FMD_ERR_DEVICE, "%s", e);
    hipLaunchKernelGGL(k_modmon<S>, dim3((unsigned)m->C), dim3(kT), 0, s, static_cast<const typename fmd::Iq<S>::raw*>(d_in), in_stride, n, d_active,
                       m->taps, m->design.hz_per_rad, m->design.M, m->design.P, m->d_pilot, m->d_status, m->d_part, m->d_carry, m->d_hist);
    if (hipGetLastError() != hipSuccess) return mm_fail(m, FMD_ERR_DEVICE, "k_modmon launch failed");
    if (const char* e = m->order.end(s)) return mm_fail(m, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

extern "C" {

int fmd_modmon_create(const fmd_modmon_config* cfg, fmd_modmon* out) {
    if (!cfg || !out) return mm_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->n_channels <= 0 || cfg->max_input_samples <= 0 || cfg->max_input_samples > (1LL << 30))
        return mm_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_samples %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_samples);
    fmd_modmon_design_t d;
    if (fmd::modmon_design(cfg->fs, &d, &fmd::modmon_global_error()) != FMD_OK) return FMD_ERR_ARG;
    if (fmd_device_count() <= 0) return mm_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return mm_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_modmon m = new fmd_modmon_s();
    m->C = cfg->n_channels; m->fs = cfg->fs; m->max_in = cfg->max_input_samples;
    m->design = d;
    for (int t = 0; t < kModmonTaps; t++) m->taps.h[t] = d.h[t];
    const size_t C = (size_t)m->C;
    bool ok = m->order.init(dev);
    ok = ok && hipMalloc(&m->d_status, sizeof(fmd_modmon_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_part, sizeof(double) * kCarryD * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_carry, sizeof(float) * kCarryF * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_hist, sizeof(unsigned) * kModmonBins * C) == hipSuccess;
    ok = ok && hipMalloc(&m->d_pilot, sizeof(double) * 2 * kModmonMaxP) == hipSuccess;
    ok = ok && hipMemcpy(m->d_pilot, d.pilot_cos, sizeof(double) * kModmonMaxP, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(m->d_pilot + kModmonMaxP, d.pilot_sin, sizeof(double) * kModmonMaxP, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok || fmd_modmon_reset(m, -1) != FMD_OK) { fmd_modmon_destroy(m); return mm_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed"); }
    *out = m;
    return FMD_OK;
}

int fmd_modmon_destroy(fmd_modmon m) {
    if (!m) return FMD_ERR_ARG;
    (void)m->order.quiesce();
    for (void* p : {(void*)m->d_status, (void*)m->d_part, (void*)m->d_carry, (void*)m->d_hist, (void*)m->d_pilot})
        if (p) (void)hipFree(p);
    delete m;
    return FMD_OK;
}

int fmd_modmon_reset(fmd_modmon m, int channel) { return mm_reset(m, channel, 0); }

int fmd_modmon_reset_peaks(fmd_modmon m, int channel) { return mm_reset(m, channel, 1); }

int fmd_modmon_process_cf32_dev(fmd_modmon m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, void* stream) {
    return mm_process<float2>(m, d_in, 8, in_stride, n, d_active, stream);
}

int fmd_modmon_process_u8_dev(fmd_modmon m, const uint8_t* d_in, long long in_stride, long long n, const uint8_t* d_active, void* stream) {
    return mm_process<uint8_t>(m, d_in, 2, in_stride, n, d_active, stream);
}

int fmd_modmon_get_status(fmd_modmon m, fmd_modmon_status* out) {
    if (!m || !out) return mm_fail(m, FMD_ERR_ARG, "null monitor or output");
    if (!m->order.quiesce()) return mm_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, m->d_status, sizeof(fmd_modmon_status) * (size_t)m->C, hipMemcpyDeviceToHost) != hipSuccess) return mm_fail(m, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_modmon_get_histogram(fmd_modmon m, unsigned* hist) {
    if (!m || !hist) return mm_fail(m, FMD_ERR_ARG, "null monitor or output");
    if (!m->order.quiesce()) return mm_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(hist, m->d_hist, sizeof(unsigned) * kModmonBins * (size_t)m->C, hipMemcpyDeviceToHost) != hipSuccess) return mm_fail(m, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_modmon_status_dev(fmd_modmon m, const fmd_modmon_status** d_status) {
    if (!m || !d_status) return mm_fail(m, FMD_ERR_ARG, "null monitor or output");
    *d_status = m->d_status;
    return FMD_OK;
}

const char* fmd_modmon_last_error(fmd_modmon m) { return m ? m->err.c_str() : fmd::modmon_global_error().c_str(); }

}  // extern "C"
