// Band scanner, device side (include/fmdemod.h, "Band scan"): the averaged periodogram of a wideband capture.
//
// NOT in the reference (its RTL-SDR hardware tunes one known station).  Definition, restated in float64 by tests/scan_ref.py:
//     frame f = absolute input samples [f H, f H + N), H = N / 2, counted since create / reset; it counts once its last sample arrives
//     P_f[k] = |sum_n w[n] x[f H + n] e^{-j 2 pi k n / N}|^2          (w: periodic Hann, fp32 values computed in double on the host)
//     S[k]   = sum_f P_f[k]                                            (fp64, in frame order)
// so S does not depend, bit for bit, on how the capture is split into calls: a frame's P_f is a function of its N samples alone (one
// workgroup, a fixed sequence of fp32 operations), and the per-bin sum runs over the frames in order whatever call delivered them.
//
// Two kernels per call, on the caller's stream:
//   * k_scan_frames: one workgroup per frame that completes in this call.  A radix-8/4 Stockham FFT in LDS (N complex fp32, 128 KB at
//     N = 16384): the first pass reads the frame's samples straight from the window [history][block], converts (Iq<S>), windows and runs
//     its radix-8 butterflies in registers; the middle passes run in place in LDS (every thread reads its butterflies' inputs, barrier,
//     writes the outputs, barrier); the last pass writes |X|^2, fft-shifted, to the frame's row of a [frames][N] fp32 scratch buffer.
//     Twiddles come from a table e^{-j 2 pi m / N} computed in double on the host and stored as fp32.  One extra workgroup hands the
//     window's unframed tail (< N samples) over to the other history buffer, which no workgroup of the launch reads.
//   * k_scan_accumulate: one thread per bin adds the call's frame rows to its fp64 sum in frame order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "fmd_iq.h"
#include "fmd_scan_design.h"
#include "fmd_side.h"
#include "fmdemod.h"

using fmd::Iq;

namespace {

// radix plan of N = 2^LOGN: radix-8 passes first, then one or two radix-4 passes (never radix 2); NT threads per workgroup
template <int LOGN> struct Plan {
    static constexpr int N = 1 << LOGN, H = N / 2;
    static constexpr int NT = N / 8 < 512 ? N / 8 : 512;
    static constexpr int N8 = LOGN % 3 == 1 ? LOGN / 3 - 1 : LOGN / 3;
    static constexpr int N4 = (LOGN - 3 * N8) / 2;
    static constexpr int PASSES = N8 + N4;
    static_assert(3 * N8 + 2 * N4 == LOGN && N8 >= 2, "radix plan");
    static constexpr int radix(int p) { return p < N8 ? 8 : 4; }
};

// the window of a call: [h_len history samples][the caller's block]; absolute index of window sample 0 = first unframed sample
template <typename S> struct ScanWin { const float2* hist; const typename Iq<S>::raw* blk; float2* next_hist; };
struct ScanDims {
    int h_len;     // history samples in front of the block
    int frames;    // frames completing in this call (workgroups 0 .. frames - 1); workgroup `frames` carries the tail over
    int n_carry;   // samples of the tail: window [frames H, h_len + n_in)
};

template <typename S>
__device__ __forceinline__ float2 win_at(const ScanWin<S>& w, int h_len, long long j) {
    if (j < h_len) return w.hist[j];
    return Iq<S>::cf32(w.blk[j - h_len]);
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mul_mj(float2 a) { return make_float2(a.y, -a.x); }   // a * (-j)

// in-place forward DFTs (e^{-j 2 pi k n / R}) of R = 4 and R = 8 values
__device__ __forceinline__ void dft4(float2* v) {
    const float2 s02 = cadd(v[0], v[2]), d02 = csub(v[0], v[2]), s13 = cadd(v[1], v[3]), d13 = mul_mj(csub(v[1], v[3]));
    v[0] = cadd(s02, s13); v[2] = csub(s02, s13);
    v[1] = cadd(d02, d13); v[3] = csub(d02, d13);
}
__device__ __forceinline__ void dft8(float2* v) {
    float2 e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
    dft4(e); dft4(o);
    constexpr float c = 0.70710678118654752f;
    o[1] = make_float2(c * (o[1].x + o[1].y), c * (o[1].y - o[1].x));      // * e^{-j pi / 4}
    o[2] = mul_mj(o[2]);                                                     // * e^{-j pi / 2}
    o[3] = make_float2(c * (o[3].y - o[3].x), -c * (o[3].x + o[3].y));     // * e^{-j 3 pi / 4}
    for (int k = 0; k < 4; k++) { v[k] = cadd(e[k], o[k]); v[k + 4] = csub(e[k], o[k]); }
}
template <int R> __device__ __forceinline__ void dft(float2* v) {
    if constexpr (R == 8) dft8(v); else dft4(v);
}

// butterfly j of a Stockham pass of radix R after sub-transforms of size NS: inputs j + r N / R, twiddled by e^{-j 2 pi r (j mod NS) / (NS R)}
template <int N, int R, int NS>
__device__ __forceinline__ void twiddle(float2* v, int j, const float2* __restrict__ tw) {
    if constexpr (NS > 1) {
        const int k = j & (NS - 1);
#pragma unroll
        for (int r = 1; r < R; r++) v[r] = cmul(v[r], tw[r * k * (N / (NS * R))]);
    }
}

// the middle passes, LDS to LDS in place: pass P of the plan, sub-transforms of size NS done
template <int LOGN, int P, int NS>
__device__ __forceinline__ void middle_passes(float2* lds, const float2* __restrict__ tw) {
    using Pl = Plan<LOGN>;
    if constexpr (P < Pl::PASSES - 1) {
        constexpr int N = Pl::N, NT = Pl::NT, R = Pl::radix(P), B = N / R / NT;
        float2 v[B][R];
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int j = threadIdx.x + b * NT;
#pragma unroll
            for (int r = 0; r < R; r++) v[b][r] = lds[j + r * (N / R)];
            twiddle<N, R, NS>(v[b], j, tw);
            dft<R>(v[b]);
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int j = threadIdx.x + b * NT, k = j & (NS - 1), o = (j - k) * R + k;
#pragma unroll
            for (int r = 0; r < R; r++) lds[o + r * NS] = v[b][r];
        }
        __syncthreads();
        middle_passes<LOGN, P + 1, NS * R>(lds, tw);
    }
}

template <int LOGN, typename S>
__global__ __launch_bounds__(Plan<LOGN>::NT) void k_scan_frames(ScanWin<S> w, ScanDims d, const float* __restrict__ window,
                                                              const float2* __restrict__ tw, float* __restrict__ power) {
    using Pl = Plan<LOGN>;
    constexpr int N = Pl::N, H = Pl::H, NT = Pl::NT;
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int f = blockIdx.x;
    if (f == d.frames) {                       // the unframed tail becomes the next call's history
        for (int i = threadIdx.x; i < d.n_carry; i += NT) w.next_hist[i] = win_at(w, d.h_len, (long long)d.frames * H + i);
        return;
    }
    const long long base = (long long)f * H;
    {   // first pass (radix 8, NS = 1): samples -> window -> butterfly -> LDS
        constexpr int B = N / 8 / NT;
        float2 v[B][8];
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int j = threadIdx.x + b * NT;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int n = j + r * (N / 8);
                const float2 x = win_at(w, d.h_len, base + n);
                const float wn = window[n];
                v[b][r] = make_float2(x.x * wn, x.y * wn);
            }
        }
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int j = threadIdx.x + b * NT;
            dft8(v[b]);
#pragma unroll
            for (int r = 0; r < 8; r++) lds[j * 8 + r] = v[b][r];
        }
        __syncthreads();
    }
    middle_passes<LOGN, 1, 8>(lds, tw);
    {   // last pass (NS = N / R): LDS -> butterfly -> |X|^2 at bin k = j + r N / R, stored at (k + N / 2) mod N
        constexpr int R = Pl::radix(Pl::PASSES - 1), NS = N / R, B = N / R / NT;
        float* row = power + (size_t)f * N;
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int j = threadIdx.x + b * NT;
            float2 v[R];
#pragma unroll
            for (int r = 0; r < R; r++) v[r] = lds[j + r * NS];
            twiddle<N, R, NS>(v, j, tw);
            dft<R>(v);
#pragma unroll
            for (int r = 0; r < R; r++) row[(j + r * NS) ^ (N / 2)] = v[r].x * v[r].x + v[r].y * v[r].y;
        }
    }
}

// S[i] += the call's frame rows, in frame order (fp64).  Loads are grouped so that 16 are in flight per thread; the adds stay in order.
__global__ __launch_bounds__(64) void k_scan_accumulate(const float* __restrict__ power, int frames, int N, double* __restrict__ acc) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    double s = acc[i];
    int f = 0;
    for (; f + 16 <= frames; f += 16) {
        float p[16];
#pragma unroll
        for (int u = 0; u < 16; u++) p[u] = power[(size_t)(f + u) * N + i];
#pragma unroll
        for (int u = 0; u < 16; u++) s += (double)p[u];
    }
    for (; f < frames; f++) s += (double)power[(size_t)f * N + i];
    acc[i] = s;
}

template <typename S> using FramesFn = void (*)(ScanWin<S>, ScanDims, const float*, const float2*, float*);
template <typename S> FramesFn<S> frames_kernel(int logn) {
    switch (logn) {
        case 8: return k_scan_frames<8, S>;
        case 9: return k_scan_frames<9, S>;
        case 10: return k_scan_frames<10, S>;
        case 11: return k_scan_frames<11, S>;
        case 12: return k_scan_frames<12, S>;
        case 13: return k_scan_frames<13, S>;
        default: return k_scan_frames<14, S>;
    }
}
static int threads_for(int logn) { return (1 << logn) / 8 < 512 ? (1 << logn) / 8 : 512; }

}  // namespace

struct fmd_scanner_s {
    int N = 0, logn = 0;
    double fs_in = 0;
    double sum_w2 = 0;                 // sum of the fp32 window values squared, in double
    size_t max_in = 0;
    int max_frames = 0;                // frames one call can complete: the scratch rows
    unsigned long long n_abs = 0;      // absolute index of the next input sample
    long long n_frames = 0;            // frames accumulated since create / reset
    int h_len = 0;                     // history samples: [n_frames H, n_abs)
    float2* hist[2] = {nullptr, nullptr};   // [N - 1] each, ping-pong: a launch reads one and writes the next call's history into the other
    int cur = 0;
    float* window = nullptr;           // [N]
    float2* tw = nullptr;              // [N] e^{-j 2 pi m / N}
    float* power = nullptr;            // [max_frames][N] scratch: the call's frame powers, fft-shifted
    double* acc = nullptr;             // [N] S, fft-shifted
    fmd::CallOrder order;              // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int scan_fail(fmd_scanner h, int code, const char* fmt, A... args) { return fmd::fail(h ? h->err : fmd::scan_global_error(), code, fmt, args...); }

template <typename S> static bool set_lds(int logn) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(frames_kernel<S>(logn)), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(sizeof(float2) << logn)) == hipSuccess;
}

template <typename S>
static int scan_process(fmd_scanner h, const void* d_wide, size_t n_in, void* stream) {
    if (!h || !d_wide) return scan_fail(h, FMD_ERR_ARG, "null scanner or input");
    if (n_in == 0 || n_in > h->max_in) return scan_fail(h, FMD_ERR_SIZE, "n_in %zu outside (0, %zu]", n_in, h->max_in);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the history and the scratch rows carry over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* e = h->order.begin(s)) return scan_fail(h, FMD_ERR_DEVICE, "%s", e);
    const int N = h->N, H = N / 2;
    const long long W = (long long)h->h_len + (long long)n_in;
    const int frames = W >= N ? (int)((W - N) / H + 1) : 0;
    ScanDims d{h->h_len, frames, (int)(W - (long long)frames * H)};
    const ScanWin<S> w{h->hist[h->cur], static_cast<const typename Iq<S>::raw*>(d_wide), h->hist[h->cur ^ 1]};
    hipLaunchKernelGGL(frames_kernel<S>(h->logn), dim3((unsigned)frames + 1), dim3(threads_for(h->logn)), sizeof(float2) * N, s, w, d,
                       h->window, h->tw, h->power);
    if (hipGetLastError() != hipSuccess) return scan_fail(h, FMD_ERR_DEVICE, "k_scan_frames launch failed");
    if (frames > 0) {
        hipLaunchKernelGGL(k_scan_accumulate, dim3((unsigned)(N / 64)), dim3(64), 0, s, h->power, frames, N, h->acc);
        if (hipGetLastError() != hipSuccess) return scan_fail(h, FMD_ERR_DEVICE, "k_scan_accumulate launch failed");
    }
    if (const char* e = h->order.end(s)) return scan_fail(h, FMD_ERR_DEVICE, "%s", e);
    h->cur ^= 1;
    h->n_abs += n_in;
    h->n_frames += frames;
    h->h_len = d.n_carry;
    return FMD_OK;
}

extern "C" {

int fmd_scan_create(const fmd_scan_config* cfg, fmd_scanner* out) {
    if (!cfg || !out) return scan_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (!(std::isfinite(cfg->fs_in) && cfg->fs_in > 0)) return scan_fail(nullptr, FMD_ERR_ARG, "fs_in %g must be finite and > 0", cfg->fs_in);
    const int N = cfg->nfft == 0 ? fmd_scan_default_nfft(cfg->fs_in) : cfg->nfft;
    if (!fmd::scan_nfft_ok(N)) return scan_fail(nullptr, FMD_ERR_ARG, "nfft %d is not a power of two in 256 ... 16384", cfg->nfft);
    if (cfg->max_input_samples <= 0 || cfg->max_input_samples > (1LL << 32))
        return scan_fail(nullptr, FMD_ERR_ARG, "max_input_samples %lld outside (0, 2^32]", cfg->max_input_samples);
    if (fmd_device_count() <= 0) return scan_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return scan_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_scanner h = new fmd_scanner_s();
    h->N = N; h->fs_in = cfg->fs_in; h->max_in = (size_t)cfg->max_input_samples;
    while ((1 << h->logn) < N) h->logn++;
    const long long wmax = (long long)(N - 1) + cfg->max_input_samples;
    h->max_frames = wmax >= N ? (int)((wmax - N) / (N / 2) + 1) : 0;
    std::vector<float> win(N);
    std::vector<float2> tw(N);
    for (int n = 0; n < N; n++) {
        win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)N));
        h->sum_w2 += (double)win[n] * (double)win[n];
        const double a = -2.0 * M_PI * (double)n / (double)N;
        tw[n] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    bool ok = h->order.init(dev);
    for (int i = 0; i < 2; i++) ok = ok && hipMalloc(&h->hist[i], sizeof(float2) * (size_t)(N - 1)) == hipSuccess;
    ok = ok && hipMalloc(&h->window, sizeof(float) * N) == hipSuccess;
    ok = ok && hipMalloc(&h->tw, sizeof(float2) * N) == hipSuccess;
    ok = ok && hipMalloc(&h->power, sizeof(float) * (size_t)N * (size_t)(h->max_frames > 0 ? h->max_frames : 1)) == hipSuccess;
    ok = ok && hipMalloc(&h->acc, sizeof(double) * N) == hipSuccess;
    ok = ok && hipMemcpy(h->window, win.data(), sizeof(float) * N, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(h->tw, tw.data(), sizeof(float2) * N, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemset(h->acc, 0, sizeof(double) * N) == hipSuccess;
    ok = ok && set_lds<float2>(h->logn) && set_lds<uint8_t>(h->logn) && set_lds<int8_t>(h->logn) && set_lds<int16_t>(h->logn);
    if (!ok) { fmd_scan_destroy(h); return scan_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed"); }
    *out = h;
    return FMD_OK;
}

int fmd_scan_destroy(fmd_scanner h) {
    if (!h) return FMD_ERR_ARG;
    (void)h->order.quiesce();
    for (int i = 0; i < 2; i++) if (h->hist[i]) (void)hipFree(h->hist[i]);
    if (h->window) (void)hipFree(h->window);
    if (h->tw) (void)hipFree(h->tw);
    if (h->power) (void)hipFree(h->power);
    if (h->acc) (void)hipFree(h->acc);
    delete h;
    return FMD_OK;
}

int fmd_scan_reset(fmd_scanner h) {
    if (!h) return FMD_ERR_ARG;
    if (!h->order.quiesce()) return scan_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemset(h->acc, 0, sizeof(double) * h->N) != hipSuccess) return scan_fail(h, FMD_ERR_DEVICE, "memset failed");
    h->n_abs = 0; h->n_frames = 0; h->h_len = 0; h->cur = 0;
    return FMD_OK;
}

int fmd_scan_process_cf32_dev(fmd_scanner h, const float* d_wide, size_t n_in, void* stream) {
    return scan_process<float2>(h, d_wide, n_in, stream);
}
int fmd_scan_process_u8_dev(fmd_scanner h, const uint8_t* d_wide, size_t n_in, void* stream) {
    return scan_process<uint8_t>(h, d_wide, n_in, stream);
}
int fmd_scan_process_s8_dev(fmd_scanner h, const int8_t* d_wide, size_t n_in, void* stream) {
    return scan_process<int8_t>(h, d_wide, n_in, stream);
}
int fmd_scan_process_s16_dev(fmd_scanner h, const int16_t* d_wide, size_t n_in, void* stream) {
    return scan_process<int16_t>(h, d_wide, n_in, stream);
}

int fmd_scan_get_psd(fmd_scanner h, double* psd, int cap, long long* n_frames) {
    if (!h || !psd) return scan_fail(h, FMD_ERR_ARG, "null scanner or output");
    if (cap < h->N) return scan_fail(h, FMD_ERR_SIZE, "capacity %d < nfft %d", cap, h->N);
    if (!h->order.quiesce()) return scan_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(psd, h->acc, sizeof(double) * h->N, hipMemcpyDeviceToHost) != hipSuccess) return scan_fail(h, FMD_ERR_DEVICE, "copy failed");
    if (h->n_frames > 0) {
        const double scale = (double)h->n_frames * h->fs_in * h->sum_w2;
        for (int i = 0; i < h->N; i++) psd[i] /= scale;
    }
    if (n_frames) *n_frames = h->n_frames;
    return FMD_OK;
}

int fmd_scan_stations(fmd_scanner h, const fmd_scan_params* p, fmd_scan_station* out, int cap, int* n_found) {
    if (!h) return scan_fail(h, FMD_ERR_ARG, "null scanner");
    std::vector<double> psd(h->N);
    const int rc = fmd_scan_get_psd(h, psd.data(), h->N, nullptr);
    if (rc != FMD_OK) return rc;
    fmd_scan_params def;
    if (!p) { fmd_scan_default_params(&def); p = &def; }
    return fmd::scan_detect(psd.data(), h->N, h->fs_in, p, out, cap, n_found, &h->err);
}

const char* fmd_scan_last_error(fmd_scanner h) { return h ? h->err.c_str() : fmd::scan_global_error().c_str(); }

}  // extern "C"
