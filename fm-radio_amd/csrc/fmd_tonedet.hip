// Audio tone detector, device side (include/fmdemod.h, "Audio tone detector").
//
// NOT in the reference.  Per station and per 100 ms interval the sum MM = sum m^2 of the mid signal m = L + R of the station audio
// [C][in_stride][2] f32 that the mixer, the loudness meter and the fault monitor read, read in place, and per used tone slot the two sums
// RE = sum m cos, IM = sum m sin against the handle's table of fs entries; at an interval's end the eight hysteresis detectors, and at a
// call's end the [C] flags and ok bytes.
//
// One kernel per call, k_tonedet, on the row walk of fmd_rows.h as k_audmon is (one wavefront per station, rows of 256 frames), with two
// rows in registers ahead.  With NP = 64 and j = (r >> 2) & 63 lane l owns exactly partial l of each of the 17 sums (34 fp64
// accumulators with the mid signal's and eight slots') and adds its four terms of a row in ascending r.  Per frame and used slot one
// 16-byte gather of (cos, sin) from the table in global memory (at most 768 KB, shared by every station: it stays in L2); the table
// index moves from frame to frame and from row to row by an add and a conditional subtract, with one modulo per slot and segment.  The
// slots are walked by an unrolled loop with a wave-uniform test per slot, so that the accumulators stay in registers.  A frame that
// reads as (+0, +0) changes no partial (fma(+0, t, s) = s for a finite t: a partial is never -0).  At an interval's end the partials
// fold by cross-lane moves in the contract's halving order, and lane 0 alone writes the ring, runs the detectors on the station's
// record and stores, with ordinary stores.  The open interval's 8.5 KB of partials are read at the call's start and written at its
// end.  No atomics, no LDS, no scratch.
//
// Denormals: fp64 and fp32 denormals are kept (hipcc's default mode; this file is NOT built with -fgpu-flush-denormals-to-zero).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fmd_rows.h"
#include "fmd_side.h"
#include "fmd_tonedet_design.h"
#include "fmdemod.h"

using fmd::kTonedetPartials;
using fmd::kTonedetRing;
using fmd::kTonedetSlots;
using fmd::kTonedetSums;
using fmd::TonedetGate;

namespace {

namespace rows = fmd::rows;
using rows::kQ;                      // frames per lane and row
using rows::kRow;                    // frames per row
using rows::kT;                      // threads per workgroup: one wavefront, one station
constexpr int kPf = 2;               // rows loaded ahead
constexpr int kPartD = kTonedetSums * kTonedetPartials;    // doubles per station: the open interval's partials
static_assert(kTonedetPartials == kT && kTonedetRing == 30 && kTonedetSlots == 8 && kTonedetSums == 17, "k_tonedet's lane layout");

static_assert(sizeof(fmd_tonedet_status) == 2344 && offsetof(fmd_tonedet_status, intervals) == 8 && offsetof(fmd_tonedet_status, intervals_flagged) == 16 &&
              offsetof(fmd_tonedet_status, ring_mm) == 80 && offsetof(fmd_tonedet_status, ring_pw) == 320 && offsetof(fmd_tonedet_status, run) == 2240 &&
              offsetof(fmd_tonedet_status, transitions) == 2272 && offsetof(fmd_tonedet_status, nonfinite) == 2304 &&
              offsetof(fmd_tonedet_status, freq_hz) == 2308 && offsetof(fmd_tonedet_status, flags) == 2340 && offsetof(fmd_tonedet_status, ok) == 2341 &&
              offsetof(fmd_tonedet_status, reserved) == 2342, "fmd_tonedet_status layout");
static_assert(sizeof(TonedetGate) == 176 && sizeof(fmd_tonedet_params) == 176, "TonedetGate and fmd_tonedet_params layout");

// a + b mod fs for a, b < fs
__device__ __forceinline__ unsigned td_step(unsigned a, unsigned b, unsigned fs) {
    const unsigned s = a + b;
    return s >= fs ? s - fs : s;
}

// in [C][in_stride] frames (L, R); tab [fs] (cos, sin); gate [C]; status [C]; part [C][17][64]; out_flags, out_ok [C] or null
__global__ __launch_bounds__(kT) void k_tonedet(const float2* __restrict__ in, long long in_stride, long long n, const uint8_t* __restrict__ active, int fs, int M,
                                                const double2* __restrict__ tab, const TonedetGate* __restrict__ gate,
                                                fmd_tonedet_status* __restrict__ status, double* __restrict__ part, uint8_t* __restrict__ out_flags,
                                                uint8_t* __restrict__ out_ok) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (active && active[c] == 0) return;                                    // (uniform over the wavefront)
    fmd_tonedet_status* st = status + c;
    const TonedetGate* gt = gate + c;                                        // (uniform)
    unsigned flags = st->flags;
    const unsigned alarm_mask = gt->alarm_mask;
    if (n == 0) {                                                            // nothing of the station changes but its bytes, which are still written
        if (lane == 0) {
            const uint8_t ok = (uint8_t)((flags & alarm_mask) == 0);
            st->ok = ok;
            if (out_flags) out_flags[c] = (uint8_t)flags;
            if (out_ok) out_ok[c] = ok;
        }
        return;
    }
    const float2* base = in + (size_t)c * (size_t)in_stride;
    double* pp = part + (size_t)c * kPartD + lane;
    const unsigned ufs = (unsigned)fs;

    const unsigned long long frames0 = st->frames;
    unsigned long long G = st->intervals;
    const int r0 = __builtin_amdgcn_readfirstlane((int)(frames0 - G * (unsigned long long)M));   // the first frame's place in its interval
    unsigned f[kTonedetSlots];                                               // the frequencies in force (uniform), 0 = unused
    double mm = pp[0], re[kTonedetSlots], im[kTonedetSlots];
#pragma unroll
    for (int k = 0; k < kTonedetSlots; k++) {
        f[k] = (unsigned)__builtin_amdgcn_readfirstlane(st->freq_hz[k]);
        re[k] = pp[(1 + 2 * k) * kTonedetPartials];
        im[k] = pp[(2 + 2 * k) * kTonedetPartials];
    }

    // per used slot the table index of the lane's first frame of the row at hand, and the step from one row to the next
    unsigned ix[kTonedetSlots], rowstep[kTonedetSlots];
    rows::walk<kPf>(base, lane, n, M, r0, make_float2(0.0f, 0.0f),
        [&](int r) {                                                         // the segment's first frame's place in its interval
#pragma unroll
            for (int k = 0; k < kTonedetSlots; k++) {
                ix[k] = 0u; rowstep[k] = 0u;
                if (f[k]) {
                    ix[k] = (f[k] * (unsigned)((r & ~(kRow - 1)) + kQ * lane)) % ufs;   // (below 2^31: f < 24000, r < 4800 + 256)
                    rowstep[k] = (f[k] * (unsigned)kRow) % ufs;
                }
            }
        },
        [&](const float2 (&v)[kQ]) {
            double m[kQ];
#pragma unroll
            for (int q = 0; q < kQ; q++) {
                m[q] = (double)v[q].x + (double)v[q].y;
                mm = fma(m[q], m[q], mm);
            }
#pragma unroll
            for (int k = 0; k < kTonedetSlots; k++) {
                if (f[k]) {                                                  // (uniform)
                    unsigned i[kQ];
                    i[0] = ix[k];
#pragma unroll
                    for (int q = 1; q < kQ; q++) i[q] = td_step(i[q - 1], f[k], ufs);
                    double2 t[kQ];
#pragma unroll
                    for (int q = 0; q < kQ; q++) t[q] = tab[i[q]];
#pragma unroll
                    for (int q = 0; q < kQ; q++) {
                        re[k] = fma(m[q], t[q].x, re[k]);
                        im[k] = fma(m[q], t[q].y, im[k]);
                    }
                    ix[k] = td_step(ix[k], rowstep[k], ufs);
                }
            }
        },
        [&](bool complete) {
            if (!complete) return;
            rows::fold(mm);
#pragma unroll
            for (int k = 0; k < kTonedetSlots; k++)
                if (f[k]) rows::fold(re[k], im[k]);
            if (lane == 0) {
                const double MM = mm;
                const int g = (int)(G % (unsigned long long)kTonedetRing);
                const bool finite = rows::finite(MM);
                st->ring_mm[g] = MM;
                if (!finite) st->nonfinite++;
                const bool usable = finite && MM > gt->min_e;
                const double ref = (double)M * MM;
#pragma unroll
                for (int k = 0; k < kTonedetSlots; k++) {
                    const double PW = f[k] ? fma(re[k], re[k], im[k] * im[k]) : 0.0;
                    st->ring_pw[k][g] = PW;
                    const bool present = f[k] != 0u && usable && rows::finite(PW) && 2.0 * PW > gt->c[k] * ref;
                    flags = rows::detect(flags, k, present, gt->raise_intervals[k], gt->clear_intervals[k], st->run[k], st->transitions[k]);
                }
#pragma unroll
                for (int k = 0; k < kTonedetSlots; k++) {
                    if (flags & (1u << k)) st->intervals_flagged[k]++;
                    st->freq_hz[k] = gt->freq_hz[k];                         // the next interval starts on the pending frequencies
                }
            }
            G++;
            mm = 0.0;
#pragma unroll
            for (int k = 0; k < kTonedetSlots; k++) {
                re[k] = 0.0; im[k] = 0.0;
                f[k] = (unsigned)__builtin_amdgcn_readfirstlane(gt->freq_hz[k]);
            }
        });

    // what the next call needs: the open interval's partials, and the record
    pp[0] = mm;
#pragma unroll
    for (int k = 0; k < kTonedetSlots; k++) {
        pp[(1 + 2 * k) * kTonedetPartials] = re[k];
        pp[(2 + 2 * k) * kTonedetPartials] = im[k];
    }
    if (lane == 0) {
        st->frames = frames0 + (unsigned long long)n;
        st->intervals = G;
        const uint8_t ok = (uint8_t)((flags & alarm_mask) == 0);
        st->flags = (unsigned char)flags;
        st->ok = ok;
        if (out_flags) out_flags[c] = (uint8_t)flags;
        if (out_ok) out_ok[c] = ok;
    }
}

// stations c0 ... as after create (everything 0, every flag clear, ok = 1), on their parameters' frequencies
__global__ __launch_bounds__(kT) void k_tonedet_reset(int c0, const TonedetGate* __restrict__ gate, fmd_tonedet_status* __restrict__ status,
                                                      double* __restrict__ part) {
    const int c = c0 + blockIdx.x, t = threadIdx.x;
    fmd_tonedet_status* st = status + c;
    unsigned* w = reinterpret_cast<unsigned*>(st);
    for (int i = t; i < (int)(sizeof(fmd_tonedet_status) / 4); i += kT) w[i] = 0u;
    for (int i = t; i < kPartD; i += kT) part[(size_t)c * kPartD + i] = 0.0;
    __syncthreads();
    if (t == 0) {
        for (int k = 0; k < kTonedetSlots; k++) st->freq_hz[k] = gate[c].freq_hz[k];
        st->ok = 1;
    }
}

// the parameters of stations c0 ...; a station with no open interval starts its next one on the new frequencies
__global__ __launch_bounds__(kT) void k_tonedet_set(int c0, int cn, int M, TonedetGate g, TonedetGate* __restrict__ gate, fmd_tonedet_status* __restrict__ status) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= cn) return;
    fmd_tonedet_status* st = status + c0 + i;
    gate[c0 + i] = g;
    if (st->frames == st->intervals * (unsigned long long)M)
        for (int k = 0; k < kTonedetSlots; k++) st->freq_hz[k] = g.freq_hz[k];
    st->ok = (unsigned char)((st->flags & g.alarm_mask) == 0);
}

}  // namespace

struct fmd_tonedet_s {
    int C = 0, fs = 0, M = 0;
    long long max_in = 0;
    std::vector<fmd_tonedet_params> params;  // [C], as set
    fmd_tonedet_status* d_status = nullptr;  // [C]
    TonedetGate* d_gate = nullptr;           // [C]
    double* d_part = nullptr;                // [C][17][64]
    double2* d_tab = nullptr;                // [fs]: cos, sin of 2 pi j / fs
    fmd::CallOrder order;                    // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int td_fail(fmd_tonedet t, int code, const char* fmt, A... args) { return fmd::fail(t ? t->err : fmd::tonedet_global_error(), code, fmt, args...); }

extern "C" {

int fmd_tonedet_create(const fmd_tonedet_config* cfg, fmd_tonedet* out) {
    if (!cfg || !out) return td_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->n_channels <= 0 || cfg->max_input_frames <= 0 || cfg->max_input_frames > (1LL << 30))
        return td_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_frames %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_frames);
    const int M = fmd::tonedet_interval(cfg->fs);
    if (M == 0) return td_fail(nullptr, FMD_ERR_ARG, "fs %d is not a multiple of 10 in 8000 ... 48000", cfg->fs);
    if (fmd_device_count() <= 0) return td_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return td_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_tonedet t = new fmd_tonedet_s();
    t->C = cfg->n_channels; t->fs = cfg->fs; t->M = M; t->max_in = cfg->max_input_frames;
    fmd_tonedet_params p{};
    fmd_tonedet_default_params(&p);
    t->params.assign((size_t)t->C, p);
    const size_t C = (size_t)t->C;
    std::vector<double> tab(2 * (size_t)t->fs);
    fmd::tonedet_table(t->fs, tab.data());
    bool ok = t->order.init(dev);
    ok = ok && hipMalloc(&t->d_status, sizeof(fmd_tonedet_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&t->d_gate, sizeof(TonedetGate) * C) == hipSuccess;
    ok = ok && hipMalloc(&t->d_part, sizeof(double) * kPartD * C) == hipSuccess;
    ok = ok && hipMalloc(&t->d_tab, sizeof(double) * tab.size()) == hipSuccess;
    ok = ok && hipMemset(t->d_gate, 0, sizeof(TonedetGate) * C) == hipSuccess;
    ok = ok && hipMemcpy(t->d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice) == hipSuccess;
    // (the reset first: set_params reads the record's flags and counters)
    if (!ok || fmd_tonedet_reset(t, -1) != FMD_OK || fmd_tonedet_set_params(t, -1, &p) != FMD_OK) {
        fmd_tonedet_destroy(t);
        return td_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed");
    }
    *out = t;
    return FMD_OK;
}

int fmd_tonedet_destroy(fmd_tonedet t) {
    if (!t) return FMD_ERR_ARG;
    (void)t->order.quiesce();
    for (void* p : {(void*)t->d_status, (void*)t->d_gate, (void*)t->d_part, (void*)t->d_tab})
        if (p) (void)hipFree(p);
    delete t;
    return FMD_OK;
}

int fmd_tonedet_reset(fmd_tonedet t, int channel) {
    if (!t) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, t->C, &c0, &cn)) return td_fail(t, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, t->C);
    if (!t->order.quiesce()) return td_fail(t, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_tonedet_reset, dim3((unsigned)cn), dim3(kT), 0, nullptr, c0, t->d_gate, t->d_status, t->d_part);
    if (const char* e = fmd::control_end("k_tonedet_reset launch failed")) return td_fail(t, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_tonedet_set_params(fmd_tonedet t, int channel, const fmd_tonedet_params* p) {
    if (!t) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, t->C, &c0, &cn)) return td_fail(t, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, t->C);
    TonedetGate g;
    if (fmd::tonedet_gate(p, t->fs, &g, &t->err) != FMD_OK) return FMD_ERR_ARG;
    if (!t->order.quiesce()) return td_fail(t, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_tonedet_set, dim3((unsigned)((cn + kT - 1) / kT)), dim3(kT), 0, nullptr, c0, cn, t->M, g, t->d_gate, t->d_status);
    if (const char* e = fmd::control_end("k_tonedet_set launch failed")) return td_fail(t, FMD_ERR_DEVICE, "%s", e);
    for (int c = c0; c < c0 + cn; c++) t->params[(size_t)c] = *p;
    return FMD_OK;
}

int fmd_tonedet_get_params(fmd_tonedet t, int channel, fmd_tonedet_params* p) {
    if (!t || !p) return td_fail(t, FMD_ERR_ARG, "null detector or output");
    if (channel < 0 || channel >= t->C) return td_fail(t, FMD_ERR_ARG, "channel %d outside [0, %d)", channel, t->C);
    *p = t->params[(size_t)channel];
    return FMD_OK;
}

int fmd_tonedet_process_f32_dev(fmd_tonedet t, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_flags, uint8_t* d_ok,
                                void* stream) {
    if (!t) return FMD_ERR_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return td_fail(t, FMD_ERR_ARG, "null input, or input not aligned to 8 bytes");
    if (n < 0 || n > in_stride || n > t->max_in)
        return td_fail(t, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or above max_input_frames %lld", n, in_stride, t->max_in);
    if (n == 0 && !d_flags && !d_ok) return FMD_OK;                          // nothing of any station changes and there is no byte to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* e = t->order.begin(s)) return td_fail(t, FMD_ERR_DEVICE, "%s", e);
    hipLaunchKernelGGL(k_tonedet, dim3((unsigned)t->C), dim3(kT), 0, s, reinterpret_cast<const float2*>(d_in), in_stride, n, d_active, t->fs, t->M, t->d_tab,
                       t->d_gate, t->d_status, t->d_part, d_flags, d_ok);
    if (hipGetLastError() != hipSuccess) return td_fail(t, FMD_ERR_DEVICE, "k_tonedet launch failed");
    if (const char* e = t->order.end(s)) return td_fail(t, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_tonedet_get_status(fmd_tonedet t, fmd_tonedet_status* out) {
    if (!t || !out) return td_fail(t, FMD_ERR_ARG, "null detector or output");
    if (!t->order.quiesce()) return td_fail(t, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, t->d_status, sizeof(fmd_tonedet_status) * (size_t)t->C, hipMemcpyDeviceToHost) != hipSuccess) return td_fail(t, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_tonedet_status_dev(fmd_tonedet t, const fmd_tonedet_status** d_status) {
    if (!t || !d_status) return td_fail(t, FMD_ERR_ARG, "null detector or output");
    *d_status = t->d_status;
    return FMD_OK;
}

const char* fmd_tonedet_last_error(fmd_tonedet t) { return t ? t->err.c_str() : fmd::tonedet_global_error().c_str(); }

}  // extern "C"
