// DC offset and IQ imbalance corrector, device side (include/fmdemod.h, "DC offset and IQ imbalance correction").
//
// NOT in the reference.  One pass over a wideband capture (cf32, u8, s8, s16): every raw sample is read once, added to five fp64 moments
// and written back as cf32, y = z + w conj(z), z = x - dc.  The moments' summation order is a function of the absolute sample index since
// reset alone (chunks of 4096, 256 partial sums per chunk, a halving tree, chunk sums in chunk order), so they do not depend, bit for bit,
// on how the capture is split into calls.
//
// Two kernels per call, on the caller's stream:
//   * k_iqcorr<S>: a group of 256 / P threads per chunk, P = the samples of one 16-byte load (cf32 2, s16 4, u8 / s8 8), P chunks per
//     workgroup of 256 threads.  Thread t of a group owns the partial sums j = P t ... P t + P - 1 of its chunk: step k loads the 16 bytes
//     of samples 256 k + P t ... (non-temporal where the address allows a 16-byte load, else sample by sample) and adds each sample's
//     terms, in double, to its partial, so every partial runs over k ascending in one thread's registers.  The same thread corrects the
//     samples in fp32 and stores them, 16 bytes at a time where the output address allows.  A chunk that an earlier call left open starts
//     from its stored partials; a chunk the call leaves open stores them; a chunk the call completes goes through the halving tree in
//     LDS and writes its five sums to the call's scratch row.
//   * k_iqcorr_fold: one workgroup adds the call's chunk sums to the running totals in chunk order (staged through LDS; lanes 0 ... 4
//     run the five chains).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "fmd_iq.h"
#include "fmd_iqcorr_design.h"
#include "fmd_side.h"
#include "fmdemod.h"

using fmd::Iq;
using fmd::kIqChunk;
using fmd::kIqLanes;
using fmd::kIqMoments;

namespace {

constexpr int kT = 256;                          // threads per workgroup
constexpr int kSteps = kIqChunk / kIqLanes;      // 16 terms per partial sum
constexpr int kU = 4;                            // steps whose loads are issued before their sums
constexpr int kFoldTile = 1024;                  // chunk sums k_iqcorr_fold holds in LDS at a time

typedef unsigned nt_u4 __attribute__((ext_vector_type(4)));
typedef float nt_f4 __attribute__((ext_vector_type(4)));

// sample e of the P raw samples in one 16-byte load
template <typename S> __device__ __forceinline__ typename Iq<S>::raw raw_at(const nt_u4& v, int e);
template <> __device__ __forceinline__ float2 raw_at<float2>(const nt_u4& v, int e) {
    return make_float2(__uint_as_float(v[2 * e]), __uint_as_float(v[2 * e + 1]));
}
template <> __device__ __forceinline__ unsigned int raw_at<int16_t>(const nt_u4& v, int e) { return v[e]; }
template <> __device__ __forceinline__ unsigned short raw_at<uint8_t>(const nt_u4& v, int e) {
    return (unsigned short)((v[e >> 1] >> (16 * (e & 1))) & 0xffffu);
}
template <> __device__ __forceinline__ unsigned short raw_at<int8_t>(const nt_u4& v, int e) { return raw_at<uint8_t>(v, e); }

// in: the call's first sample, absolute index a; n samples.  open_rd [5][256]: the partials of the chunk the previous call left open;
// open_wr: those of the chunk this call leaves open (another buffer: the call's first and last chunk may run in any order);
// sums [chunks of the call][5].  in and out may be the same array (cf32): no __restrict__ on them.
template <typename S>
__global__ __launch_bounds__(kT) void k_iqcorr(const typename Iq<S>::raw* in, long long a, long long n, float* out, fmd_iq_correction cr,
                                               const double* __restrict__ open_rd, double* __restrict__ open_wr, double* __restrict__ sums, int vec_in,
                                               int vec_out) {
    using raw_t = typename Iq<S>::raw;
    constexpr int P = 16 / (int)sizeof(raw_t);   // samples per 16-byte load = partial sums per thread = chunks per workgroup
    constexpr int G = kIqLanes / P;              // threads per chunk
    extern __shared__ __attribute__((aligned(16))) double red[];   // [P chunks][5][256]
    const int tid = threadIdx.x, g = tid / G, tl = tid % G;
    const long long c0 = a / kIqChunk;                               // the call's first chunk
    const long long base = (c0 + (long long)blockIdx.x * P + g) * kIqChunk;
    const long long lo = base > a ? base : a;
    const long long hi = base + kIqChunk < a + n ? base + kIqChunk : a + n;   // the chunk's samples in this call: [lo, hi), empty past the call's end
    double acc[P][kIqMoments];
#pragma unroll
    for (int e = 0; e < P; e++)
#pragma unroll
        for (int m = 0; m < kIqMoments; m++) acc[e][m] = (hi > lo && base < a) ? open_rd[m * kIqLanes + P * tl + e] : 0.0;
    if (hi > lo) {
        for (int k0 = 0; k0 < kSteps; k0 += kU) {
            raw_t r[kU][P];
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const long long s0 = base + (long long)(k0 + u) * kIqLanes + P * tl;
                if (vec_in && s0 >= lo && s0 + P <= hi) {
                    const nt_u4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_u4*>(in + (s0 - a)));
#pragma unroll
                    for (int e = 0; e < P; e++) r[u][e] = raw_at<S>(v, e);
                } else {
#pragma unroll
                    for (int e = 0; e < P; e++) r[u][e] = (s0 + e >= lo && s0 + e < hi) ? in[s0 + e - a] : Iq<S>::zero();
                }
            }
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const long long s0 = base + (long long)(k0 + u) * kIqLanes + P * tl;
                float2 y[P];
#pragma unroll
                for (int e = 0; e < P; e++) {
                    // a sample outside [lo, hi) reads as (+0, +0): its terms are +0 and leave the partial's bits as they are
                    const float2 x = Iq<S>::cf32(r[u][e]);
                    const double di = (double)x.x, dq = (double)x.y;
                    acc[e][0] += di;
                    acc[e][1] += dq;
                    acc[e][2] += di * di;
                    acc[e][3] += dq * dq;
                    acc[e][4] += di * dq;
                    const float zi = x.x - cr.dc_i, zq = x.y - cr.dc_q;
                    y[e] = make_float2(fmaf(cr.w_re, zi, fmaf(cr.w_im, zq, zi)), fmaf(cr.w_im, zi, fmaf(-cr.w_re, zq, zq)));
                }
                if (!out) continue;
                if (vec_out && s0 >= lo && s0 + P <= hi) {
                    nt_f4* o = reinterpret_cast<nt_f4*>(out + 2 * (s0 - a));
#pragma unroll
                    for (int e = 0; e < P; e += 2) o[e / 2] = nt_f4{y[e].x, y[e].y, y[e + 1].x, y[e + 1].y};
                } else {
#pragma unroll
                    for (int e = 0; e < P; e++)
                        if (s0 + e >= lo && s0 + e < hi) *reinterpret_cast<float2*>(out + 2 * (s0 + e - a)) = y[e];
                }
            }
        }
        if (hi < base + kIqChunk) {                // the call leaves the chunk open (only its last chunk can be)
#pragma unroll
            for (int e = 0; e < P; e++)
#pragma unroll
                for (int m = 0; m < kIqMoments; m++) open_wr[m * kIqLanes + P * tl + e] = acc[e][m];
        }
    }
#pragma unroll
    for (int e = 0; e < P; e++)
#pragma unroll
        for (int m = 0; m < kIqMoments; m++) red[(g * kIqMoments + m) * kIqLanes + P * tl + e] = acc[e][m];
    __syncthreads();
    // the halving tree of the workgroup's P x 5 rows of 256 partials
    for (int h = kIqLanes / 2; h >= 1; h >>= 1) {
        for (int idx = tid; idx < P * kIqMoments * h; idx += kT) {
            const int row = idx / h, j = idx - row * h;
            red[row * kIqLanes + j] += red[row * kIqLanes + j + h];
        }
        __syncthreads();
    }
    if (tid < P * kIqMoments) {
        const long long cc = (long long)blockIdx.x * P + tid / kIqMoments;     // the row's chunk, counted from c0
        if ((c0 + cc + 1) * kIqChunk <= a + n) sums[cc * kIqMoments + tid % kIqMoments] = red[tid * kIqLanes];
    }
}

// total[m] += sums[c][m] for c = 0 ... n_chunks - 1, in that order
__global__ __launch_bounds__(kT) void k_iqcorr_fold(const double* __restrict__ sums, int n_chunks, double* __restrict__ total) {
    __shared__ double tile[kFoldTile * kIqMoments];
    const int tid = threadIdx.x;
    double t = tid < kIqMoments ? total[tid] : 0.0;
    for (int c0 = 0; c0 < n_chunks; c0 += kFoldTile) {
        const int cnt = n_chunks - c0 < kFoldTile ? n_chunks - c0 : kFoldTile;
        for (int i = tid; i < cnt * kIqMoments; i += kT) tile[i] = sums[(size_t)c0 * kIqMoments + i];
        __syncthreads();
        if (tid < kIqMoments)
            for (int c = 0; c < cnt; c++) t += tile[c * kIqMoments + tid];
        __syncthreads();
    }
    if (tid < kIqMoments) total[tid] = t;
}

template <typename S> constexpr int lds_bytes() {
    return (16 / (int)sizeof(typename Iq<S>::raw)) * kIqMoments * kIqLanes * (int)sizeof(double);
}
template <typename S> bool set_lds() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_iqcorr<S>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes<S>()) == hipSuccess;
}

}  // namespace

struct fmd_iqcorr_s {
    long long max_in = 0;
    unsigned long long n_abs = 0;      // samples since create / reset: the absolute index of the next one
    fmd_iq_correction corr{0.f, 0.f, 0.f, 0.f};
    double* total = nullptr;           // [5] sums of the completed chunks
    double* open[2] = {nullptr, nullptr};   // [5][256] each, ping-pong: a launch reads the open chunk's partials from one and writes the
    int cur = 0;                       // next call's into the other; open[cur] is valid while n_abs is no multiple of 4096
    double* sums = nullptr;            // [max_in / 4096 + 2][5] scratch: the chunk sums of one call
    fmd::CallOrder order;              // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int iq_fail(fmd_iqcorr h, int code, const char* fmt, A... args) { return fmd::fail(h ? h->err : fmd::iqcorr_global_error(), code, fmt, args...); }

template <typename S>
static int iq_process(fmd_iqcorr h, const void* d_in, long long n_in, float* d_out, void* stream) {
    using raw_t = typename Iq<S>::raw;
    constexpr int P = 16 / (int)sizeof(raw_t);
    if (!h) return iq_fail(h, FMD_ERR_ARG, "null corrector");
    if (!d_in) return iq_fail(h, FMD_ERR_ARG, "null input");
    if (n_in <= 0 || n_in > h->max_in) return iq_fail(h, FMD_ERR_ARG, "n_in %lld outside (0, %lld]", n_in, h->max_in);
    const uintptr_t pi = reinterpret_cast<uintptr_t>(d_in), po = reinterpret_cast<uintptr_t>(d_out);
    if (pi % sizeof(raw_t) != 0 || po % sizeof(float2) != 0) return iq_fail(h, FMD_ERR_ARG, "d_in is not aligned to an I / Q pair or d_out not to 8 bytes");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the totals, the open chunk and the scratch row carry over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* e = h->order.begin(s)) return iq_fail(h, FMD_ERR_DEVICE, "%s", e);
    const unsigned long long a = h->n_abs, end = a + (unsigned long long)n_in;
    const long long c0 = (long long)(a / kIqChunk), c1 = (long long)((end - 1) / kIqChunk);
    const int touched = (int)(c1 - c0 + 1), closed = (int)((long long)(end / kIqChunk) - c0);
    // sample s of the capture sits at d_in + (s - a): 16-byte loads and stores are aligned when the address of absolute sample 0 is
    const int vec_in = (pi + 16 - (a * sizeof(raw_t)) % 16) % 16 == 0;
    const int vec_out = (po + 16 - (a * sizeof(float2)) % 16) % 16 == 0;
    hipLaunchKernelGGL(k_iqcorr<S>, dim3((unsigned)((touched + P - 1) / P)), dim3(kT), lds_bytes<S>(), s, static_cast<const raw_t*>(d_in),
                       (long long)a, n_in, d_out, h->corr, h->open[h->cur], h->open[h->cur ^ 1], h->sums, vec_in, vec_out);
    if (hipGetLastError() != hipSuccess) return iq_fail(h, FMD_ERR_DEVICE, "k_iqcorr launch failed");
    if (closed > 0) {
        hipLaunchKernelGGL(k_iqcorr_fold, dim3(1), dim3(kT), 0, s, h->sums, closed, h->total);
        if (hipGetLastError() != hipSuccess) return iq_fail(h, FMD_ERR_DEVICE, "k_iqcorr_fold launch failed");
    }
    if (const char* e = h->order.end(s)) return iq_fail(h, FMD_ERR_DEVICE, "%s", e);
    h->cur ^= 1;
    h->n_abs = end;
    return FMD_OK;
}

extern "C" {

int fmd_iqcorr_create(const fmd_iqcorr_config* cfg, fmd_iqcorr* out) {
    if (!cfg || !out) return iq_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->max_input_samples <= 0 || cfg->max_input_samples > (1LL << 32))
        return iq_fail(nullptr, FMD_ERR_ARG, "max_input_samples %lld outside (0, 2^32]", cfg->max_input_samples);
    if (fmd_device_count() <= 0) return iq_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return iq_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_iqcorr h = new fmd_iqcorr_s();
    h->max_in = cfg->max_input_samples;
    const size_t rows = (size_t)(h->max_in / kIqChunk) + 2;
    bool ok = h->order.init(dev);
    ok = ok && hipMalloc(&h->total, sizeof(double) * kIqMoments) == hipSuccess;
    for (int i = 0; i < 2; i++) ok = ok && hipMalloc(&h->open[i], sizeof(double) * kIqMoments * kIqLanes) == hipSuccess;
    ok = ok && hipMalloc(&h->sums, sizeof(double) * kIqMoments * rows) == hipSuccess;
    ok = ok && hipMemset(h->total, 0, sizeof(double) * kIqMoments) == hipSuccess;
    ok = ok && set_lds<float2>() && set_lds<uint8_t>() && set_lds<int8_t>() && set_lds<int16_t>();
    if (!ok) { fmd_iqcorr_destroy(h); return iq_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed"); }
    *out = h;
    return FMD_OK;
}

int fmd_iqcorr_destroy(fmd_iqcorr h) {
    if (!h) return FMD_ERR_ARG;
    (void)h->order.quiesce();
    if (h->total) (void)hipFree(h->total);
    for (int i = 0; i < 2; i++) if (h->open[i]) (void)hipFree(h->open[i]);
    if (h->sums) (void)hipFree(h->sums);
    delete h;
    return FMD_OK;
}

int fmd_iqcorr_reset_moments(fmd_iqcorr h) {
    if (!h) return FMD_ERR_ARG;
    if (!h->order.quiesce()) return iq_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemset(h->total, 0, sizeof(double) * kIqMoments) != hipSuccess) return iq_fail(h, FMD_ERR_DEVICE, "memset failed");
    h->n_abs = 0;
    return FMD_OK;
}

int fmd_iqcorr_reset(fmd_iqcorr h) {
    const int rc = fmd_iqcorr_reset_moments(h);
    if (rc != FMD_OK) return rc;
    h->corr = fmd_iq_correction{0.f, 0.f, 0.f, 0.f};
    return FMD_OK;
}

int fmd_iqcorr_process_cf32_dev(fmd_iqcorr h, const float* d_in, long long n_in, float* d_out, void* stream) {
    return iq_process<float2>(h, d_in, n_in, d_out, stream);
}
int fmd_iqcorr_process_u8_dev(fmd_iqcorr h, const uint8_t* d_in, long long n_in, float* d_out, void* stream) {
    return iq_process<uint8_t>(h, d_in, n_in, d_out, stream);
}
int fmd_iqcorr_process_s8_dev(fmd_iqcorr h, const int8_t* d_in, long long n_in, float* d_out, void* stream) {
    return iq_process<int8_t>(h, d_in, n_in, d_out, stream);
}
int fmd_iqcorr_process_s16_dev(fmd_iqcorr h, const int16_t* d_in, long long n_in, float* d_out, void* stream) {
    return iq_process<int16_t>(h, d_in, n_in, d_out, stream);
}

int fmd_iqcorr_get_moments(fmd_iqcorr h, fmd_iq_moments* out) {
    if (!h || !out) return iq_fail(h, FMD_ERR_ARG, "null corrector or output");
    if (!h->order.quiesce()) return iq_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    double t[kIqMoments];
    if (hipMemcpy(t, h->total, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess) return iq_fail(h, FMD_ERR_DEVICE, "copy failed");
    if (h->n_abs % kIqChunk != 0) {            // the open chunk: its tree on a copy, the device's partials stay as they are
        double p[kIqMoments * kIqLanes];
        if (hipMemcpy(p, h->open[h->cur], sizeof(p), hipMemcpyDeviceToHost) != hipSuccess) return iq_fail(h, FMD_ERR_DEVICE, "copy failed");
        for (int m = 0; m < kIqMoments; m++) t[m] += fmd::iqcorr_tree(p + m * kIqLanes);
    }
    *out = fmd_iq_moments{(double)h->n_abs, t[0], t[1], t[2], t[3], t[4]};
    return FMD_OK;
}

int fmd_iqcorr_set_correction(fmd_iqcorr h, const fmd_iq_correction* c) {
    if (!h || !c) return iq_fail(h, FMD_ERR_ARG, "null corrector or correction");
    if (!fmd::iqcorr_finite(*c)) return iq_fail(h, FMD_ERR_ARG, "the correction is not finite");
    h->corr = *c;
    return FMD_OK;
}

int fmd_iqcorr_get_correction(fmd_iqcorr h, fmd_iq_correction* c) {
    if (!h || !c) return iq_fail(h, FMD_ERR_ARG, "null corrector or output");
    *c = h->corr;
    return FMD_OK;
}

int fmd_iqcorr_calibrate(fmd_iqcorr h, fmd_iq_correction* out) {
    if (!h) return iq_fail(h, FMD_ERR_ARG, "null corrector");
    fmd_iq_moments m;
    int rc = fmd_iqcorr_get_moments(h, &m);
    if (rc != FMD_OK) return rc;
    fmd_iq_correction c;
    rc = fmd::iqcorr_solve(&m, &c, &h->err);
    if (rc != FMD_OK) return rc;
    h->corr = c;
    if (out) *out = c;
    return FMD_OK;
}

const char* fmd_iqcorr_last_error(fmd_iqcorr h) { return h ? h->err.c_str() : fmd::iqcorr_global_error().c_str(); }

}  // extern "C"
