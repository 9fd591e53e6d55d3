// Log-mel front end, device side (include/fmdemod.h, "Log-mel front end").
//
// NOT in the reference.  Per station the mono signal m = 0.5f (L + R) of the station audio [C][in_stride][2] f32 that the mixer and the
// monitors read, read in place; per completed window of N samples the windowed DFT's K bins as two fmaf chains in ascending n, their
// powers, the mel bands as fmaf chains in ascending k, and the logarithm: rows of n_mels f32 for a model.
//
// One kernel per call, k_logmel: one workgroup of four wavefronts per station.  The window, the (cos, sin) table and, pass by pass, the
// mono samples of up to 16 spectral frames lie in LDS (at most 64 KB: fmd_logmel_design.cpp's layout takes fewer frames a pass where N
// and K are large).  The DFT of a pass is a GEMM on the matrix cores: v_mfma_f32_16x16x4_f32 with spectral frames as rows, bins as
// columns and the depth running over n in ascending order through the accumulator from a zero C, which is a k-ordered fmaf chain with
// one rounding per product.  The A operand xw = w[n] * m[t hop + n] is formed where it is read; the B operand is gathered from the
// N-entry table in LDS, one 8-byte read of (cos, sin) per lane and step feeding the re and the im MFMA, with the index (k n) mod N moved
// by an add and a conditional subtract.  A wavefront owns up to four 16-bin tiles at a time (eight independent accumulators) and shares
// the A operand among them.  The powers go to LDS as P [frame][Kp], zero from K on; the mel GEMM takes them as its A operand against the
// filterbank image fbT [Kp][Mp] in global memory (it stays in L2), and the epilogue applies flog10 and stores the rows.  The samples
// from the next uncompleted window's start on go back to the object through LDS.  No atomics, no scratch, no workgroup waits on another.
//
// A VALU form of the same kernel (every lane its four frames x one bin or band of a tile, explicit fmaf in the same order) was built as
// the fallback, gave the same bytes and took 2.6 x the time; it is not kept.
//
// Bounds: every LDS index lies inside the layout's regions (rows are clamped to the pass's last row, bins run below Kp <= N / 2 + 16,
// table indices below N); global reads of the input lie below n <= in_stride, of the carry below N; rows are stored for frames below the
// call's count <= fmd_logmel_max_frames(hop, n) and bands below n_mels, inside out_stride.
//
// Denormals: fp32 denormals are kept (hipcc's default mode; this file is NOT built with -fgpu-flush-denormals-to-zero).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fmd_logmel_design.h"
#include "fmd_logmel_math.h"
#include "fmd_side.h"
#include "fmdemod.h"

using fmd::kLogmelTile;
using fmd::LogmelLayout;

namespace {

constexpr int kT = 256;              // threads per workgroup: four wavefronts, one station
constexpr int kWaves = kT / 64;
constexpr int kNB = 4;               // bin tiles a wavefront works on at once
constexpr int kMB = 2;               // band tiles a wavefront works on at once (Mp <= 128: eight tiles over four wavefronts)
static_assert(kLogmelTile == 16, "the 16x16x4 MFMA's tile");

static_assert(sizeof(fmd_logmel_status) == 32 && offsetof(fmd_logmel_status, spectra) == 8 && offsetof(fmd_logmel_status, nonfinite) == 16 &&
              offsetof(fmd_logmel_status, fill) == 24 && offsetof(fmd_logmel_status, reserved) == 28, "fmd_logmel_status layout");

typedef float lm_f4 __attribute__((ext_vector_type(4)));

// what the kernel reads of the configuration and the layout
struct LogmelDev {
    int N, hop, n_mels, K, Kp, Mp, rows, span;
    int off_tab, off_m, off_p, off_nf;
    int out_mode;
    float floor;
};

// a + b mod N for a, b < N
__device__ __forceinline__ int lm_step(int a, int b, int N) {
    const int s = a + b;
    return s >= N ? s - N : s;
}

// sample q of the station's stream counted from the next uncompleted window's start: kept ones first, then the call's
__device__ __forceinline__ float lm_sample(const float* __restrict__ carry, const float2* __restrict__ in, long long q, long long fill) {
    if (q < fill) return carry[q];
    const float2 v = in[q - fill];
    return 0.5f * (v.x + v.y);
}

// in [C][in_stride] frames (L, R); w [N]; tab [N] (cos, sin); fbT [Kp][Mp]; status [C]; carry [C][N]; out [C][out_stride]; nframes [C] or null
__global__ __launch_bounds__(kT) void k_logmel(const float2* __restrict__ in, long long in_stride, long long n, const uint8_t* __restrict__ active, LogmelDev g,
                                               const float* __restrict__ d_w, const float2* __restrict__ d_tab, const float* __restrict__ fbT,
                                               fmd_logmel_status* __restrict__ status, float* __restrict__ carry_all, float* __restrict__ out,
                                               long long out_stride, int* __restrict__ nframes) {
    extern __shared__ float lds[];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (active && active[c] == 0) return;                                    // (uniform over the workgroup)
    const int N = g.N, hop = g.hop;
    float* s_w = lds;
    float2* s_tab = reinterpret_cast<float2*>(lds + g.off_tab);
    float* s_m = lds + g.off_m;
    float* s_p = lds + g.off_p;
    int* s_nf = reinterpret_cast<int*>(lds + g.off_nf);

    fmd_logmel_status* st = status + c;
    const unsigned long long frames0 = st->frames, T0 = st->spectra;
    const long long fill = (long long)st->fill;
    const unsigned long long total = frames0 + (unsigned long long)n;
    const unsigned long long T1 = fmd::logmel_spectra(total, N, hop);
    const int nsp = (int)(T1 - T0);                                          // spectral frames of this call, at most (n + hop - 1) / hop
    const long long avail = fill + n;                                        // samples at hand from frame T0's start on
    const float2* base = in + (size_t)c * (size_t)in_stride;
    float* carry = carry_all + (size_t)c * (size_t)N;
    float* orow = out + (size_t)c * (size_t)out_stride;

    for (int i = tid; i < N; i += kT) { s_w[i] = d_w[i]; s_tab[i] = d_tab[i]; }
    int mynf = 0;                                                            // threads 0 ... 15: the non-finite frames of their row

    const int col = lane & 15, kq = lane >> 4;
    const int ntiles = g.Kp / kLogmelTile;
    const int tpw = min(kNB, (ntiles + kWaves - 1) / kWaves);                // bin tiles of a group
    const int mtiles = g.Mp / kLogmelTile;

    for (int tb = 0; tb < nsp; tb += g.rows) {
        const int rv = min(g.rows, nsp - tb);                                // the pass's spectral frames
        const long long q0 = (long long)tb * hop;
        __syncthreads();                                                     // the pass before is done with m, P and the flags
        for (int i = tid; i < g.span; i += kT) {
            const long long q = q0 + i;
            s_m[i] = q < avail ? lm_sample(carry, base, q, fill) : 0.0f;
        }
        if (tid < kLogmelTile) s_nf[tid] = 0;
        __syncthreads();

        // ---- the DFT and the powers: groups of tpw bin tiles, round robin over the wavefronts
        for (int t0 = wave * tpw; t0 < ntiles; t0 += kWaves * tpw) {
            const int cnt = min(tpw, ntiles - t0);
            lm_f4 re[kNB], im[kNB];
            int idx[kNB], stp[kNB];
#pragma unroll
            for (int j = 0; j < kNB; j++) {
                re[j] = lm_f4{0.0f, 0.0f, 0.0f, 0.0f}; im[j] = re[j];
                const int k = (min(t0 + j, ntiles - 1)) * kLogmelTile + col;
                idx[j] = (k * kq) % N;
                stp[j] = (4 * k) % N;
            }
            const float* am = s_m + min(col, g.rows - 1) * hop + kq;     // the A operand's row of samples (a row past the pass repeats its last)
            const float* aw = s_w + kq;
            for (int n0 = 0; n0 < N; n0 += 4) {
                const float a = aw[n0] * am[n0];                         // xw: one rounding
#pragma unroll
                for (int j = 0; j < kNB; j++) {
                    if (j < cnt) {                                       // (uniform)
                        const float2 t = s_tab[idx[j]];
                        re[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, t.x, re[j], 0, 0, 0);
                        im[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, t.y, im[j], 0, 0, 0);
                        idx[j] = lm_step(idx[j], stp[j], N);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kNB; j++) {
                if (j < cnt) {
                    const int k = (t0 + j) * kLogmelTile + col;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int row = kq * 4 + r;
                        if (row < g.rows) s_p[row * g.Kp + k] = k < g.K ? fmaf(re[j][r], re[j][r], im[j][r] * im[j][r]) : 0.0f;
                    }
                }
            }
        }
        __syncthreads();

        // ---- the mel bands, the logarithm and the rows: pairs of band tiles, round robin over the wavefronts
        for (int b0 = wave * kMB; b0 < mtiles; b0 += kWaves * kMB) {
            const int cnt = min(kMB, mtiles - b0);
            lm_f4 mel[kMB];
#pragma unroll
            for (int j = 0; j < kMB; j++) mel[j] = lm_f4{0.0f, 0.0f, 0.0f, 0.0f};
            const float* ap = s_p + min(col, g.rows - 1) * g.Kp + kq;
            const float* bp = fbT + (size_t)kq * (size_t)g.Mp + (size_t)(b0 * kLogmelTile + col);
            for (int k0 = 0; k0 < g.Kp; k0 += 4) {
                const float a = ap[k0];
#pragma unroll
                for (int j = 0; j < kMB; j++)
                    if (j < cnt) mel[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[(size_t)k0 * (size_t)g.Mp + j * kLogmelTile], mel[j], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < kMB; j++) {
                const int band = (b0 + j) * kLogmelTile + col;
                if (j < cnt && band < g.n_mels) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int row = kq * 4 + r;
                        if (row < rv) {
                            const float v = fmd::logmel_out(mel[j][r], g.out_mode, g.floor);
                            orow[(size_t)(tb + row) * (size_t)g.n_mels + (size_t)band] = v;
                            if ((fmd::lm_f32_bits(v) & 0x7f800000u) == 0x7f800000u) s_nf[row] = 1;   // +-inf or NaN (every writer stores 1)
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (tid < kLogmelTile) mynf += s_nf[tid];
    }

    // ---- what the next call needs: the samples from the next uncompleted window's start on, through LDS (a thread's sample may be
    // another thread's target), and the record
    const long long shift = (long long)nsp * hop;
    const int newfill = (int)(avail - shift);                                // 0 ... N - 1
    __syncthreads();
    for (int i = tid; i < newfill; i += kT) s_m[i] = lm_sample(carry, base, shift + i, fill);
    if (tid < kLogmelTile) s_nf[tid] = mynf;
    __syncthreads();
    for (int i = tid; i < newfill; i += kT) carry[i] = s_m[i];
    if (tid == 0) {
        int bad = 0;
        for (int i = 0; i < kLogmelTile; i++) bad += s_nf[i];
        st->frames = total;
        st->spectra = T1;
        st->nonfinite += (unsigned long long)bad;
        st->fill = (unsigned)newfill;
        if (nframes) nframes[c] = nsp;
    }
}

// stations c0 ... as after create
__global__ __launch_bounds__(64) void k_logmel_reset(int c0, int cn, fmd_logmel_status* __restrict__ status) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= cn) return;
    fmd_logmel_status z{};
    status[c0 + i] = z;
}

}  // namespace

struct fmd_logmel_s {
    fmd_logmel_config cfg{};
    LogmelLayout lay{};
    LogmelDev dev{};
    fmd_logmel_status* d_status = nullptr;   // [C]
    float* d_carry = nullptr;                // [C][N]: the kept mono samples
    float* d_w = nullptr;                    // [N]
    float2* d_tab = nullptr;                 // [N]: cos, sin of 2 pi j / N
    float* d_fbT = nullptr;                  // [Kp][Mp]: the filterbank, bins down, zero in the padding
    fmd::CallOrder order;                    // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int lm_fail(fmd_logmel h, int code, const char* fmt, A... args) { return fmd::fail(h ? h->err : fmd::logmel_global_error(), code, fmt, args...); }

extern "C" {

int fmd_logmel_create(const fmd_logmel_config* cfg, fmd_logmel* out) {
    if (!cfg || !out) return lm_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    std::string why;
    if (fmd::logmel_check(cfg, &why) != FMD_OK) return lm_fail(nullptr, FMD_ERR_ARG, "%s", why.c_str());
    if (fmd_device_count() <= 0) return lm_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return lm_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_logmel h = new fmd_logmel_s();
    h->cfg = *cfg;
    h->lay = fmd::logmel_layout(cfg);
    const LogmelLayout& L = h->lay;
    h->dev = LogmelDev{cfg->win, cfg->hop, cfg->n_mels, L.K, L.Kp, L.Mp, L.rows, L.span, L.off_tab, L.off_m, L.off_p, L.off_nf, cfg->out_mode, cfg->log_floor};
    const size_t N = (size_t)cfg->win, C = (size_t)cfg->n_channels;
    std::vector<float> w(N), tc(N), ts(N), fb((size_t)cfg->n_mels * (size_t)L.K), tab(2 * N), fbT((size_t)L.Kp * (size_t)L.Mp, 0.0f);
    if (fmd_logmel_design(cfg, w.data(), tc.data(), ts.data(), fb.data(), nullptr) != FMD_OK) { delete h; return FMD_ERR_ARG; }
    for (size_t j = 0; j < N; j++) { tab[2 * j] = tc[j]; tab[2 * j + 1] = ts[j]; }
    for (int j = 0; j < cfg->n_mels; j++)
        for (int k = 0; k < L.K; k++) fbT[(size_t)k * (size_t)L.Mp + (size_t)j] = fb[(size_t)j * (size_t)L.K + (size_t)k];
    bool ok = h->order.init(dev);
    ok = ok && hipMalloc(&h->d_status, sizeof(fmd_logmel_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&h->d_carry, sizeof(float) * N * C) == hipSuccess;
    ok = ok && hipMalloc(&h->d_w, sizeof(float) * N) == hipSuccess;
    ok = ok && hipMalloc(&h->d_tab, sizeof(float) * tab.size()) == hipSuccess;
    ok = ok && hipMalloc(&h->d_fbT, sizeof(float) * fbT.size()) == hipSuccess;
    ok = ok && hipMemset(h->d_carry, 0, sizeof(float) * N * C) == hipSuccess;
    ok = ok && hipMemcpy(h->d_w, w.data(), sizeof(float) * N, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(h->d_tab, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(h->d_fbT, fbT.data(), sizeof(float) * fbT.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok || fmd_logmel_reset(h, -1) != FMD_OK) {
        fmd_logmel_destroy(h);
        return lm_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed");
    }
    *out = h;
    return FMD_OK;
}

int fmd_logmel_destroy(fmd_logmel h) {
    if (!h) return FMD_ERR_ARG;
    (void)h->order.quiesce();
    for (void* p : {(void*)h->d_status, (void*)h->d_carry, (void*)h->d_w, (void*)h->d_tab, (void*)h->d_fbT})
        if (p) (void)hipFree(p);
    delete h;
    return FMD_OK;
}

int fmd_logmel_reset(fmd_logmel h, int channel) {
    if (!h) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, h->cfg.n_channels, &c0, &cn)) return lm_fail(h, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, h->cfg.n_channels);
    if (!h->order.quiesce()) return lm_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_logmel_reset, dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, nullptr, c0, cn, h->d_status);
    if (const char* e = fmd::control_end("k_logmel_reset launch failed")) return lm_fail(h, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_logmel_process_f32_dev(fmd_logmel h, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, float* d_out, long long out_stride,
                               int* d_nframes, void* stream) {
    if (!h) return FMD_ERR_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return lm_fail(h, FMD_ERR_ARG, "null input, or input not aligned to 8 bytes");
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 4 != 0) return lm_fail(h, FMD_ERR_ARG, "null output, or output not aligned to 4 bytes");
    if (n < 0 || n > in_stride || n > h->cfg.max_input_frames)
        return lm_fail(h, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or above max_input_frames %lld", n, in_stride, h->cfg.max_input_frames);
    const long long need = fmd_logmel_max_frames(h->cfg.hop, n) * (long long)h->cfg.n_mels;
    if (out_stride < need) return lm_fail(h, FMD_ERR_ARG, "out_stride %lld below the %lld floats the call may write", out_stride, need);
    if (n == 0 && !d_nframes) return FMD_OK;                                 // nothing of any station changes and there is no count to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* e = h->order.begin(s)) return lm_fail(h, FMD_ERR_DEVICE, "%s", e);
    const size_t lds = sizeof(float) * (size_t)h->lay.total;
    hipLaunchKernelGGL(k_logmel, dim3((unsigned)h->cfg.n_channels), dim3(kT), lds, s, reinterpret_cast<const float2*>(d_in), in_stride, n, d_active, h->dev, h->d_w,
                       h->d_tab, h->d_fbT, h->d_status, h->d_carry, d_out, out_stride, d_nframes);
    if (hipGetLastError() != hipSuccess) return lm_fail(h, FMD_ERR_DEVICE, "k_logmel launch failed");
    if (const char* e = h->order.end(s)) return lm_fail(h, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_logmel_get_status(fmd_logmel h, fmd_logmel_status* out) {
    if (!h || !out) return lm_fail(h, FMD_ERR_ARG, "null object or output");
    if (!h->order.quiesce()) return lm_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, h->d_status, sizeof(fmd_logmel_status) * (size_t)h->cfg.n_channels, hipMemcpyDeviceToHost) != hipSuccess)
        return lm_fail(h, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_logmel_status_dev(fmd_logmel h, const fmd_logmel_status** d_status) {
    if (!h || !d_status) return lm_fail(h, FMD_ERR_ARG, "null object or output");
    *d_status = h->d_status;
    return FMD_OK;
}

const char* fmd_logmel_last_error(fmd_logmel h) { return h ? h->err.c_str() : fmd::logmel_global_error().c_str(); }

}  // extern "C"
