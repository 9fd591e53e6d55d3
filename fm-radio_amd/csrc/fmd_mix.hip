// Batched audio mixer (include/fmdemod.h "Batched audio mixer"): the reference's AudioMixer::UpdateMixer
// (src/audio/audio_mixer.cpp:33-79) for B buses at once, reading station audio that is already on the device.
//
// Every output value is one fp32 chain acc = fmaf(x_k, scale, acc) over the bus's delivering sources in registration order, run by one
// lane, so outputs do not depend on the tiling, the batch or the kernel.  The host computes scale per (bus, delivering count)
// (fmd_mix_design.cpp); the device counts the delivering sources and looks the scale up.
//
// Denormals: this file is compiled with -fgpu-flush-denormals-to-zero (Makefile), so the kernels start with MODE.FP_DENORM's f32 field
// = 0 (".amdhsa_float_denorm_mode_32 0" in the code object): v_fma_f32 then reads denormal inputs as zeros of their sign and writes
// denormal results as zeros of their sign, which is what the reference's MXCSR (FTZ + DAZ from crtfastmath) does.  DESIGN.md §6c.
//
// Two kernels, chosen per bus from its size (a call launches each for the buses it serves):
//   k_mix_stream  buses of fewer than kStagedMin sources (the reference app's own shape: one station, clamp(gain x)): one thread per two
//                 frames and tile, 16-byte loads and non-temporal stores, the bus's sources walked in order with a wave-uniform skip of
//                 the silent ones.  Streaming at the copy roof needs nothing more.
//   k_mix_staged  buses of kStagedMin sources or more (a monitoring mix): one value's chain cannot be split, and a 4800-frame block has
//                 only 9600 values, so the memory parallelism comes from the workgroup: 8 waves gather the next stages' source slices
//                 (two stages of kStS sources in registers, one in LDS) while wave 0's lanes, one per value, run the ordered chains out of
//                 LDS.  The bus's delivering sources are first compacted, in order, into an LDS list.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "fmdemod.h"
#include "fmd_mix_design.h"
#include "fmd_side.h"

namespace {

constexpr int kStagedMin = 256;      // bus size from which k_mix_staged serves a bus (measured crossover: DESIGN.md §6c)
constexpr int kStreamT = 256;        // k_mix_stream: threads per workgroup
constexpr int kStreamU = 2;          //   frame pairs per thread (kStreamT pairs apart)
constexpr int kStT = 512;            // k_mix_staged: threads per workgroup
constexpr int kStF = 32;             //   frames per workgroup (64 values: one per lane of wave 0)
constexpr int kStS = 128;            //   sources per stage (32 KB of LDS)
constexpr int kStR = kStS * kStF / kStT;   //   frames each thread gathers per stage
constexpr int kStList = 4096;        //   compacted source rows held in LDS at a time
constexpr int kChainU = 32;          //   chain steps per batch of LDS reads

__device__ __forceinline__ float clamp_ref(float acc) {
    const float t = (-1.0f > acc) ? -1.0f : acc;     // vmaxss: acc when unordered
    return (t < 1.0f) ? t : 1.0f;                    // vminss: 1 when unordered
}

// The bus's delivering-source count.  Threads of a workgroup agree on it (every thread walks the same list).
__device__ __forceinline__ int count_delivering(const int* __restrict__ rows, int k0, int k1, const uint8_t* __restrict__ active) {
    if (!active) return k1 - k0;
    int cnt = 0;
    for (int k = k0; k < k1; k++) cnt += active[rows[k]] != 0;
    return cnt;
}

// P = 2: frame pairs (in_stride, out_stride even, 16-byte aligned arrays); P = 1: single frames (any stride)
template <int P>
__global__ __launch_bounds__(kStreamT) void k_mix_stream(const float* __restrict__ in, long long in_stride, long long n,
                                                         const uint8_t* __restrict__ active, const int* __restrict__ rows,
                                                         const int* __restrict__ offs, const float* __restrict__ scales,
                                                         const int* __restrict__ bus_ids, int tiles, float* __restrict__ out,
                                                         long long out_stride) {
    const int b = bus_ids[blockIdx.x / tiles];
    const long long tile = blockIdx.x % tiles;
    const int k0 = offs[b], k1 = offs[b + 1];
    const int cnt = count_delivering(rows, k0, k1, active);
    float acc[kStreamU][2 * P];
#pragma unroll
    for (int u = 0; u < kStreamU; u++)
#pragma unroll
        for (int j = 0; j < 2 * P; j++) acc[u][j] = 0.0f;
    long long f[kStreamU];
#pragma unroll
    for (int u = 0; u < kStreamU; u++) f[u] = ((tile * kStreamU + u) * kStreamT + threadIdx.x) * P;
    if (cnt > 0) {
        const float s = scales[k0 + b + cnt];
        for (int k = k0; k < k1; k++) {
            const int r = rows[k];
            if (active && !active[r]) continue;              // wave-uniform
            const float* x = in + (size_t)r * (size_t)in_stride * 2;
            float v[kStreamU][2 * P];
#pragma unroll
            for (int u = 0; u < kStreamU; u++) {
                const long long fc = f[u] < n ? f[u] : 0;    // (a tail lane reads frame 0 and stores nothing)
                if (P == 2 && fc + 1 < n) {
                    const float4 q = *reinterpret_cast<const float4*>(x + 2 * fc);
                    v[u][0] = q.x; v[u][1] = q.y; v[u][2 % (2 * P)] = q.z; v[u][3 % (2 * P)] = q.w;
                } else {
                    const float2 q = *reinterpret_cast<const float2*>(x + 2 * fc);
                    v[u][0] = q.x; v[u][1] = q.y;
                    if (P == 2) { v[u][2 % (2 * P)] = 0.0f; v[u][3 % (2 * P)] = 0.0f; }
                }
            }
#pragma unroll
            for (int u = 0; u < kStreamU; u++)
#pragma unroll
                for (int j = 0; j < 2 * P; j++) acc[u][j] = fmaf(v[u][j], s, acc[u][j]);
        }
#pragma unroll
        for (int u = 0; u < kStreamU; u++)
#pragma unroll
            for (int j = 0; j < 2 * P; j++) acc[u][j] = clamp_ref(acc[u][j]);
    }
    float* y = out + (size_t)b * (size_t)out_stride * 2;
#pragma unroll
    for (int u = 0; u < kStreamU; u++) {
        if (f[u] >= n) continue;
        if (P == 2 && f[u] + 1 < n) {
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            const f32x4 q = {acc[u][0], acc[u][1], acc[u][2 % (2 * P)], acc[u][3 % (2 * P)]};
            __builtin_nontemporal_store(q, reinterpret_cast<f32x4*>(y + 2 * f[u]));
        } else {
            y[2 * f[u]] = acc[u][0];
            y[2 * f[u] + 1] = acc[u][1];
        }
    }
}

__global__ __launch_bounds__(kStT) void k_mix_staged(const float* __restrict__ in, long long in_stride, long long n,
                                                     const uint8_t* __restrict__ active, const int* __restrict__ rows,
                                                     const int* __restrict__ offs, const float* __restrict__ scales,
                                                     const int* __restrict__ bus_ids, int tiles, float* __restrict__ out,
                                                     long long out_stride) {
    __shared__ float xs[2][kStS * 2 * kStF];       // [buffer][source][frame][channel]
    __shared__ int list[kStList];                  // delivering source rows, in order
    __shared__ int wave_cnt[kStT / 64];
    const int b = bus_ids[blockIdx.x / tiles];
    const long long f0 = (long long)(blockIdx.x % tiles) * kStF;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k0 = offs[b], k1 = offs[b + 1];
    // the delivering count: one pass over the bus when its list does not fit in one compaction
    int cnt = k1 - k0;
    if (active && k1 - k0 > kStList) {
        cnt = 0;
        for (int k = k0; k < k1; k += kStT) cnt += __syncthreads_count(k + tid < k1 && active[rows[k + tid]] != 0);
    }
    const long long fr = f0 + (tid & (kStF - 1));  // the frame this thread gathers
    const long long frc = fr < n ? fr : n - 1;     // (gathers stay inside the row; values past n are not stored)
    const float* xin = in + (size_t)frc * 2;
    float acc = 0.0f;
    float s = 0.0f;
    bool have_scale = false;
    for (int c0 = k0; c0 < k1; c0 += kStList) {
        // ordered compaction of rows[c0 .. c0 + kStList) into list[0 .. m)
        const int c1 = (k1 - c0 < kStList) ? k1 : c0 + kStList;
        int m = 0;
        for (int k = c0; k < c1; k += kStT) {
            const bool on = k + tid < c1 && (!active || active[rows[k + tid]] != 0);
            const unsigned long long bal = __ballot(on);
            if (lane == 0) wave_cnt[wave] = __popcll(bal);
            __syncthreads();
            int before = m;
            for (int w = 0; w < wave; w++) before += wave_cnt[w];
            if (on) list[before + __popcll(bal & ((1ull << lane) - 1))] = rows[k + tid];
            for (int w = 0; w < kStT / 64; w++) m += wave_cnt[w];
            __syncthreads();
        }
        if (!have_scale) {
            if (active && k1 - k0 <= kStList) cnt = m;
            if (cnt == 0) break;
            s = scales[k0 + b + cnt];
            have_scale = true;
        }
        if (m == 0) continue;
        // stages of kStS list entries: thread t gathers frame t % kStF of sources t / kStF + (kStT / kStF) r, r < kStR
        const int nst = (m + kStS - 1) / kStS;
        float2 ra[kStR], rb[kStR];
        auto gather = [&](float2 (&g)[kStR], int st) {
            st = st < nst ? st : nst - 1;              // (past the end: a repeat of the last stage, never used)
#pragma unroll
            for (int r = 0; r < kStR; r++) {
                int k = st * kStS + tid / kStF + (kStT / kStF) * r;
                k = k < m ? k : m - 1;
                g[r] = *reinterpret_cast<const float2*>(xin + (size_t)list[k] * (size_t)in_stride * 2);
            }
        };
        auto stash = [&](const float2 (&g)[kStR], int buf) {
#pragma unroll
            for (int r = 0; r < kStR; r++)
                *reinterpret_cast<float2*>(&xs[buf][(tid / kStF + (kStT / kStF) * r) * 2 * kStF + 2 * (tid & (kStF - 1))]) = g[r];
        };
        auto chain = [&](int buf, int st) {
            if (wave != 0) return;
            const int ks = (m - st * kStS < kStS) ? m - st * kStS : kStS;
            const float* x = &xs[buf][lane];
            int k = 0;
            for (; k + kChainU <= ks; k += kChainU) {      // the reads of kChainU steps in flight ahead of their FMAs
                float v[kChainU];
#pragma unroll
                for (int u = 0; u < kChainU; u++) v[u] = x[(k + u) * 2 * kStF];
#pragma unroll
                for (int u = 0; u < kChainU; u++) acc = fmaf(v[u], s, acc);
            }
            for (; k < ks; k++) acc = fmaf(x[k * 2 * kStF], s, acc);
        };
        gather(ra, 0);
        gather(rb, 1);
        for (int st = 0; st < nst; st += 2) {
            stash(ra, 0);
            __syncthreads();
            gather(ra, st + 2);
            chain(0, st);
            if (st + 1 < nst) {
                stash(rb, 1);
                __syncthreads();
                gather(rb, st + 3);
                chain(1, st + 1);
            }
        }
        __syncthreads();                               // list and xs are rewritten by the next compaction
    }
    if (wave != 0) return;
    const long long fv = f0 + (lane >> 1);
    if (fv < n) out[(size_t)b * (size_t)out_stride * 2 + (size_t)(f0 * 2 + lane)] = have_scale ? clamp_ref(acc) : 0.0f;
}

thread_local std::string g_mix_error;

}  // namespace

struct fmd_mixer_s {
    int C = 0, B = 0;
    std::vector<std::vector<int>> sources;     // per bus, registration order
    std::vector<float> gains;
    // device tables, rebuilt from the host state before the next call after a change
    bool dirty = true;
    std::vector<int> h_rows, h_offs, h_small, h_large;
    std::vector<float> h_scales;               // bus b's entry for k delivering sources at h_offs[b] + b + k (k = 0 unused)
    int* d_rows = nullptr; int* d_offs = nullptr; int* d_small = nullptr; int* d_large = nullptr; float* d_scales = nullptr;
    size_t cap_rows = 0, cap_small = 0, cap_large = 0;
    // host-destination calls
    float* scratch = nullptr;
    size_t scratch_values = 0;
    fmd::CallOrder order;                      // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int mx_fail(fmd_mixer m, int code, const char* fmt, A... args) { return fmd::fail(m ? m->err : g_mix_error, code, fmt, args...); }

static void mx_free(fmd_mixer m) {
    for (void* p : {(void*)m->d_rows, (void*)m->d_offs, (void*)m->d_small, (void*)m->d_large, (void*)m->d_scales})
        if (p) (void)hipFree(p);
    m->d_rows = m->d_offs = m->d_small = m->d_large = nullptr; m->d_scales = nullptr;
    m->cap_rows = m->cap_small = m->cap_large = 0;
}

static bool mx_valid_sources(const fmd_mixer_s* m, const int* src, long long k) {
    if (k > 0 && !src) return false;
    for (long long i = 0; i < k; i++) if (src[i] < 0 || src[i] >= m->C) return false;
    return true;
}

// host tables -> device, in `s`'s order; the caller has quiesced (no earlier call still reads the tables)
static int mx_upload(fmd_mixer m, hipStream_t s) {
    m->h_rows.clear(); m->h_offs.assign(1, 0); m->h_small.clear(); m->h_large.clear(); m->h_scales.clear();
    for (int b = 0; b < m->B; b++) {
        const auto& v = m->sources[b];
        m->h_rows.insert(m->h_rows.end(), v.begin(), v.end());
        m->h_offs.push_back((int)m->h_rows.size());
        m->h_scales.push_back(0.0f);
        for (size_t k = 1; k <= v.size(); k++) m->h_scales.push_back(fmd::mix_scale(m->gains[b], (int)k));
        ((int)v.size() >= kStagedMin ? m->h_large : m->h_small).push_back(b);
    }
    const size_t nr = m->h_rows.size() > 0 ? m->h_rows.size() : 1;
    if (nr > m->cap_rows || m->h_small.size() > m->cap_small || m->h_large.size() > m->cap_large || !m->d_offs) {
        mx_free(m);
        const size_t ns = m->h_small.size() > 0 ? m->h_small.size() : 1, nl = m->h_large.size() > 0 ? m->h_large.size() : 1;
        if (hipMalloc(&m->d_rows, sizeof(int) * nr) != hipSuccess || hipMalloc(&m->d_offs, sizeof(int) * (size_t)(m->B + 1)) != hipSuccess ||
            hipMalloc(&m->d_small, sizeof(int) * ns) != hipSuccess || hipMalloc(&m->d_large, sizeof(int) * nl) != hipSuccess ||
            hipMalloc(&m->d_scales, sizeof(float) * (nr + (size_t)m->B)) != hipSuccess) {
            mx_free(m);
            return mx_fail(m, FMD_ERR_DEVICE, "mixer table allocation failed");
        }
        m->cap_rows = nr; m->cap_small = ns; m->cap_large = nl;
    }
    auto put = [&](void* d, const void* h, size_t bytes) { return bytes == 0 || hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s) == hipSuccess; };
    if (!put(m->d_rows, m->h_rows.data(), sizeof(int) * m->h_rows.size()) || !put(m->d_offs, m->h_offs.data(), sizeof(int) * m->h_offs.size()) ||
        !put(m->d_small, m->h_small.data(), sizeof(int) * m->h_small.size()) || !put(m->d_large, m->h_large.data(), sizeof(int) * m->h_large.size()) ||
        !put(m->d_scales, m->h_scales.data(), sizeof(float) * m->h_scales.size()))
        return mx_fail(m, FMD_ERR_DEVICE, "mixer table upload failed");
    m->dirty = false;
    return FMD_OK;
}

static int mx_process(fmd_mixer m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, float* d_out, long long out_stride,
                      hipStream_t s) {
    if (!m) return FMD_ERR_ARG;
    if (!d_in || !d_out) return mx_fail(m, FMD_ERR_ARG, "null input or output");
    if (n < 0 || n > in_stride || out_stride < n) return mx_fail(m, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or out_stride %lld < n", n, in_stride, out_stride);
    if (const char* e = m->order.begin(s)) return mx_fail(m, FMD_ERR_DEVICE, "%s", e);
    if (m->dirty) {
        if (!m->order.quiesce()) return mx_fail(m, FMD_ERR_DEVICE, "synchronise failed");
        const int rc = mx_upload(m, s);
        if (rc != FMD_OK) return rc;
    }
    if (n > 0) {
        if (!m->h_small.empty()) {
            const bool pairs = in_stride % 2 == 0 && out_stride % 2 == 0 && reinterpret_cast<uintptr_t>(d_in) % 16 == 0 &&
                               reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
            const long long per_block = (long long)kStreamT * kStreamU * (pairs ? 2 : 1);
            const int tiles = (int)((n + per_block - 1) / per_block);
            const unsigned grid = (unsigned)(tiles * (long long)m->h_small.size());
            if (pairs)
                hipLaunchKernelGGL(k_mix_stream<2>, dim3(grid), dim3(kStreamT), 0, s, d_in, in_stride, n, d_active, m->d_rows, m->d_offs, m->d_scales,
                                   m->d_small, tiles, d_out, out_stride);
            else
                hipLaunchKernelGGL(k_mix_stream<1>, dim3(grid), dim3(kStreamT), 0, s, d_in, in_stride, n, d_active, m->d_rows, m->d_offs, m->d_scales,
                                   m->d_small, tiles, d_out, out_stride);
        }
        if (!m->h_large.empty()) {
            const int tiles = (int)((n + kStF - 1) / kStF);
            hipLaunchKernelGGL(k_mix_staged, dim3((unsigned)(tiles * (long long)m->h_large.size())), dim3(kStT), 0, s, d_in, in_stride, n, d_active,
                               m->d_rows, m->d_offs, m->d_scales, m->d_large, tiles, d_out, out_stride);
        }
        if (hipGetLastError() != hipSuccess) return mx_fail(m, FMD_ERR_DEVICE, "mixer launch failed");
    }
    if (const char* e = m->order.end(s)) return mx_fail(m, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

extern "C" {

int fmd_mixer_create(const fmd_mixer_config* cfg, fmd_mixer* out) {
    if (!cfg || !out || cfg->n_channels <= 0 || cfg->n_buses <= 0 || !cfg->bus_offsets || cfg->bus_offsets[0] != 0)
        return mx_fail(nullptr, FMD_ERR_ARG, "bad mixer configuration");
    for (int b = 0; b < cfg->n_buses; b++)
        if (cfg->bus_offsets[b + 1] < cfg->bus_offsets[b]) return mx_fail(nullptr, FMD_ERR_ARG, "bus_offsets decrease at bus %d", b);
    const int total = cfg->bus_offsets[cfg->n_buses];
    fmd_mixer_s probe; probe.C = cfg->n_channels;
    if (!mx_valid_sources(&probe, cfg->bus_sources, total)) return mx_fail(nullptr, FMD_ERR_ARG, "a bus source lies outside [0, %d)", cfg->n_channels);
    if (fmd_device_count() <= 0) return mx_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return mx_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_mixer m = new fmd_mixer_s();
    m->C = cfg->n_channels; m->B = cfg->n_buses;
    m->sources.resize(m->B);
    m->gains.assign(m->B, 1.0f);
    for (int b = 0; b < m->B; b++) {
        m->sources[b].assign(cfg->bus_sources + cfg->bus_offsets[b], cfg->bus_sources + cfg->bus_offsets[b + 1]);
        if (cfg->gains) m->gains[b] = cfg->gains[b];
    }
    if (!m->order.init(dev)) {
        fmd_mixer_destroy(m);
        return mx_fail(nullptr, FMD_ERR_DEVICE, "device setup failed");
    }
    *out = m;
    return FMD_OK;
}

int fmd_mixer_destroy(fmd_mixer m) {
    if (!m) return FMD_ERR_ARG;
    (void)m->order.quiesce();
    mx_free(m);
    if (m->scratch) (void)hipFree(m->scratch);
    delete m;
    return FMD_OK;
}

int fmd_mixer_set_sources(fmd_mixer m, int bus, const int* sources, int n_sources) {
    if (!m) return FMD_ERR_ARG;
    if (bus < 0 || bus >= m->B || n_sources < 0) return mx_fail(m, FMD_ERR_ARG, "bus %d outside [0, %d) or negative source count", bus, m->B);
    if (!mx_valid_sources(m, sources, n_sources)) return mx_fail(m, FMD_ERR_ARG, "a source lies outside [0, %d)", m->C);
    m->sources[bus].assign(sources, sources + n_sources);
    m->dirty = true;
    return FMD_OK;
}

int fmd_mixer_set_gain(fmd_mixer m, int bus, float gain) {
    if (!m) return FMD_ERR_ARG;
    if (bus < -1 || bus >= m->B) return mx_fail(m, FMD_ERR_ARG, "bus %d outside [-1, %d)", bus, m->B);
    for (int b = 0; b < m->B; b++) if (bus < 0 || b == bus) m->gains[b] = gain;
    m->dirty = true;
    return FMD_OK;
}

int fmd_mixer_get_gain(fmd_mixer m, int bus, float* gain) {
    if (!m || !gain) return FMD_ERR_ARG;
    if (bus < 0 || bus >= m->B) return mx_fail(m, FMD_ERR_ARG, "bus %d outside [0, %d)", bus, m->B);
    *gain = m->gains[bus];
    return FMD_OK;
}

int fmd_mixer_process_f32_dev(fmd_mixer m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, float* d_out,
                              long long out_stride, void* stream) {
    return mx_process(m, d_in, in_stride, n, d_active, d_out, out_stride, static_cast<hipStream_t>(stream));
}

int fmd_mixer_process_f32_host(fmd_mixer m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, float* out,
                               long long out_stride, void* stream) {
    if (!m) return FMD_ERR_ARG;
    if (!d_in || !out) return mx_fail(m, FMD_ERR_ARG, "null input or output");
    if (n < 0 || n > in_stride || out_stride < n) return mx_fail(m, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or out_stride %lld < n", n, in_stride, out_stride);
    const size_t need = (size_t)m->B * (size_t)(n > 0 ? n : 1) * 2;
    if (need > m->scratch_values) {
        if (!m->order.quiesce()) return mx_fail(m, FMD_ERR_DEVICE, "synchronise failed");
        if (m->scratch) (void)hipFree(m->scratch);
        m->scratch = nullptr; m->scratch_values = 0;
        if (hipMalloc(&m->scratch, sizeof(float) * need) != hipSuccess) return mx_fail(m, FMD_ERR_DEVICE, "scratch allocation failed");
        m->scratch_values = need;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = mx_process(m, d_in, in_stride, n, d_active, m->scratch, n > 0 ? n : 1, s);
    if (rc != FMD_OK) return rc;
    if (n > 0 && hipMemcpy2DAsync(out, sizeof(float) * 2 * (size_t)out_stride, m->scratch, sizeof(float) * 2 * (size_t)n, sizeof(float) * 2 * (size_t)n,
                                  (size_t)m->B, hipMemcpyDeviceToHost, s) != hipSuccess)
        return mx_fail(m, FMD_ERR_DEVICE, "copy to the host failed");
    if (hipStreamSynchronize(s) != hipSuccess) return mx_fail(m, FMD_ERR_DEVICE, "synchronise failed");
    return FMD_OK;
}

const char* fmd_mixer_last_error(fmd_mixer m) { return m ? m->err.c_str() : g_mix_error.c_str(); }

}  // extern "C"
