// Batched audio resampler (include/fmdemod.h "Batched audio resampler"): the reference's Resampled_PCM_Player
// (src/audio/resampled_pcm_player.cpp) for C stations at once, fed with the demodulator's audio views.
//
// Both methods are memory-bound (4096 stations x 2048 frames in, 3072 out: 67 MB read, 101 MB written a 64 ms block):
//   k_resample_ref   one thread per output frame and kStations stations; the frame's (j0, w0, k) entry of the host-built index
//                    table (fmd_resample_design.cpp) is read once and used for every station; f0 / f1 are 8-byte frame loads that
//                    consecutive lanes take from (nearly) consecutive frames.  out = fmaf(f1, k, f0 * w0), the reference's order.
//   k_resample_poly  workgroup = (256 consecutive output frames, kStations stations); the input span they need
//                    (256 M / L + T frames; the first tile of a call patches the T - 1 history frames in) is staged in LDS, each
//                    thread computes one output frame of every station of the group with its phase's T taps read from the
//                    L2-resident [L][T] table, one accumulator per value, t = 0 .. T - 1 in order.  The first tile column also
//                    writes the next call's history into the other history buffer (ping-pong, as the channeliser does).
// Outputs are written with non-temporal stores (nothing reads them back on the GPU before the consumer does).
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "fmdemod.h"
#include "fmd_resample_design.h"
#include "fmd_side.h"

namespace {

constexpr int kTile = 256;            // output frames per workgroup
constexpr int kStations = 4;          // stations per workgroup
constexpr int kMaxWin = 2048;         // staged input frames per station (64 KB of LDS at most: no opt-in attribute needed)
constexpr int kDefaultTaps = 32;     // per phase, times ceil(M / L): a decimator's transition band scales with its output rate

int default_taps(int L, int M) { return kDefaultTaps * ((M + L - 1) / L); }
constexpr size_t kMaxTables = 32;     // reference-method index tables kept on the device (one per input length)

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void store_frame(float2* out, size_t i, float l, float r) {
    f32x2 v = {l, r};
    __builtin_nontemporal_store(v, reinterpret_cast<f32x2*>(out) + i);
}
// the scraper's conversion (fm_scraper.cpp:79-82), as k_audio_pcm16 does it
__device__ __forceinline__ void store_frame(short2* out, size_t i, float l, float r) {
    const float scale = 32767.0f * 0.95f;
    const unsigned int lo = (unsigned short)(short)(int)__fmul_rn(l, scale), hi = (unsigned short)(short)(int)__fmul_rn(r, scale);
    __builtin_nontemporal_store(lo | (hi << 16), reinterpret_cast<unsigned int*>(out) + i);
}

template <typename OutT>
__global__ __launch_bounds__(256) void k_resample_copy(const float2* __restrict__ in, long long in_stride, long long n, OutT* __restrict__ out,
                                                       long long out_stride, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int s = 0; s < kStations; s++) {
        const int c = blockIdx.y * kStations + s;
        if (c >= C) break;
        const float2 x = in[(size_t)c * in_stride + i];
        store_frame(out, (size_t)c * out_stride + i, x.x, x.y);
    }
}

template <typename OutT>
__global__ __launch_bounds__(256) void k_resample_ref(const float2* __restrict__ in, long long in_stride, int n_in,
                                                      const int4* __restrict__ tab /* fmd::ResampleRefTap [n_out] */, int n_out,
                                                      OutT* __restrict__ out, long long out_stride, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int4 e = tab[i];
    const int j0 = e.x, j1 = (j0 + 1 < n_in) ? j0 + 1 : j0;     // the host checked j0 < n_in
    const float w0 = __int_as_float(e.y), k = __int_as_float(e.z);
    for (int s = 0; s < kStations; s++) {
        const int c = blockIdx.y * kStations + s;
        if (c >= C) break;
        const float2* x = in + (size_t)c * in_stride;
        const float2 f0 = x[j0], f1 = x[j1];
        store_frame(out, (size_t)c * out_stride + i, fmaf(f1.x, k, __fmul_rn(f0.x, w0)), fmaf(f1.y, k, __fmul_rn(f0.y, w0)));
    }
}

struct PolyDims {
    int L, M, T, C;
    int tile, win;                    // output frames per workgroup, staged frames per station
    long long n_in, in_stride, n_out, out_stride;
    long long o0, n_abs;              // absolute index of the call's first output / first input frame
};

// input frame m (absolute, m >= n_abs - (T - 1)) of channel c: the history buffer holds [n_abs - (T - 1), n_abs)
__device__ __forceinline__ float2 poly_frame(const PolyDims& d, const float2* __restrict__ in, const float2* __restrict__ hist, int c, long long m) {
    return (m < d.n_abs) ? hist[(size_t)c * (d.T - 1) + (size_t)(m - d.n_abs + (d.T - 1))] : in[(size_t)c * d.in_stride + (size_t)(m - d.n_abs)];
}

template <typename OutT>
__global__ __launch_bounds__(256) void k_resample_poly(PolyDims d, const float2* __restrict__ in, const float2* __restrict__ hist,
                                                       float2* __restrict__ next_hist, const float* __restrict__ taps /* [L][T] */,
                                                       OutT* __restrict__ out) {
    extern __shared__ float2 xs[];    // [kStations][win]
    const int c0 = blockIdx.y * kStations, tid = threadIdx.x;
    if (blockIdx.x == 0) {
        // the next call's history: the last T - 1 frames of [history ++ this call's input]
        const long long m0 = d.n_abs + d.n_in - (d.T - 1);
        for (int s = 0; s < kStations && c0 + s < d.C; s++)
            for (int i = tid; i < d.T - 1; i += 256) next_hist[(size_t)(c0 + s) * (d.T - 1) + i] = poly_frame(d, in, hist, c0 + s, m0 + i);
    }
    const long long tile0 = (long long)blockIdx.x * d.tile;
    const int n_tile = (int)((d.n_out - tile0) < d.tile ? (d.n_out - tile0) : d.tile);
    if (n_tile <= 0) return;          // (a call that emits nothing still hands its history over)
    const long long o_first = d.o0 + tile0, o_last = o_first + n_tile - 1;
    const long long m_lo = (o_first * d.M) / d.L - (d.T - 1), n_win = (o_last * d.M) / d.L - m_lo + 1;   // <= win (host)
    for (int s = 0; s < kStations; s++) {
        const int c = c0 + s;
        for (int i = tid; i < n_win; i += 256) xs[s * d.win + i] = (c < d.C) ? poly_frame(d, in, hist, c, m_lo + i) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    if (tid >= n_tile) return;
    const long long om = (o_first + tid) * d.M;
    const int n0 = (int)(om / d.L - m_lo), p = (int)(om % d.L);
    const float* h = taps + (size_t)p * d.T;
    float al[kStations], ar[kStations];
#pragma unroll
    for (int s = 0; s < kStations; s++) { al[s] = 0.f; ar[s] = 0.f; }
    for (int t = 0; t < d.T; t += 4) {
        const float4 h4 = *reinterpret_cast<const float4*>(h + t);  // T % 4 == 0
        const float hv[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int s = 0; s < kStations; s++) {
                const float2 x = xs[s * d.win + n0 - t - u];
                al[s] = fmaf(hv[u], x.x, al[s]); ar[s] = fmaf(hv[u], x.y, ar[s]);
            }
    }
#pragma unroll
    for (int s = 0; s < kStations; s++)
        if (c0 + s < d.C) store_frame(out, (size_t)(c0 + s) * d.out_stride + (size_t)(tile0 + tid), al[s], ar[s]);
}

thread_local std::string g_rs_error;

}  // namespace

struct fmd_resampler_s {
    int C = 0, fs_in = 0, fs_out = 0, method = 0, T = 0, T_cfg = 0;   // T_cfg: the configuration's taps_per_phase (0 = default)
    long long max_in = 0;
    // polyphase
    int L = 1, M = 1, tile = kTile, win = 0;
    float* taps = nullptr;                     // [L][T]
    float2* hist[2] = {nullptr, nullptr};      // [C][T - 1] each: a launch reads one and writes the next call's into the other
    int cur = 0;
    long long n_abs = 0, o_abs = 0;            // input frames consumed / output frames emitted since the last reset
    // reference method: index tables by input length
    struct Table { int n_out = 0; int4* dev = nullptr; std::vector<fmd::ResampleRefTap> host; };
    std::map<long long, Table> tables;
    // host-destination calls
    float2* scratch = nullptr;
    size_t scratch_frames = 0;
    fmd::CallOrder order;                      // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int rs_fail(fmd_resampler r, int code, const char* fmt, A... args) { return fmd::fail(r ? r->err : g_rs_error, code, fmt, args...); }

static void rs_free_tables(fmd_resampler r) {
    for (auto& kv : r->tables) if (kv.second.dev) (void)hipFree(kv.second.dev);
    r->tables.clear();
}

// (re)design the polyphase filter for r->fs_in -> r->fs_out and clear the histories and counters; the caller has quiesced
static int rs_setup_poly(fmd_resampler r) {
    std::vector<float> h;
    int L = 0, M = 0;
    if (!fmd::resample_poly_design(r->fs_in, r->fs_out, 8, nullptr, &L, &M))
        return rs_fail(r, FMD_ERR_ARG, "unsupported polyphase rates %d -> %d", r->fs_in, r->fs_out);
    const int T = r->T_cfg > 0 ? r->T_cfg : default_taps(L, M);
    if (T != r->T || !r->hist[0]) {
        for (int i = 0; i < 2; i++) {
            if (r->hist[i]) (void)hipFree(r->hist[i]);
            r->hist[i] = nullptr;
            if (hipMalloc(&r->hist[i], sizeof(float2) * (size_t)r->C * (T - 1)) != hipSuccess) return rs_fail(r, FMD_ERR_DEVICE, "history allocation failed");
        }
        r->T = T;
    }
    if (!fmd::resample_poly_design(r->fs_in, r->fs_out, r->T, &h, &L, &M))
        return rs_fail(r, FMD_ERR_ARG, "unsupported polyphase rates %d -> %d with %d taps per phase", r->fs_in, r->fs_out, r->T);
    int tile = kTile;
    while (tile > 1 && (long long)(tile - 1) * M / L + r->T + 1 > kMaxWin) tile /= 2;
    if ((long long)(tile - 1) * M / L + r->T + 1 > kMaxWin) return rs_fail(r, FMD_ERR_ARG, "decimation %d / %d needs a larger staging window", M, L);
    std::vector<float> ph((size_t)L * r->T);                      // [t][p] -> [p][t]
    for (int t = 0; t < r->T; t++)
        for (int p = 0; p < L; p++) ph[(size_t)p * r->T + t] = h[(size_t)t * L + p];
    if (r->taps) { (void)hipFree(r->taps); r->taps = nullptr; }
    bool ok = hipMalloc(&r->taps, sizeof(float) * ph.size()) == hipSuccess &&
              hipMemcpy(r->taps, ph.data(), sizeof(float) * ph.size(), hipMemcpyHostToDevice) == hipSuccess;
    for (int i = 0; i < 2; i++) ok = ok && hipMemset(r->hist[i], 0, sizeof(float2) * (size_t)r->C * (r->T - 1)) == hipSuccess;
    if (!ok) return rs_fail(r, FMD_ERR_DEVICE, "polyphase table upload failed");
    r->L = L; r->M = M; r->tile = tile;
    r->win = (int)((long long)(tile - 1) * M / L + r->T + 1);
    r->n_abs = 0; r->o_abs = 0; r->cur = 0;
    return FMD_OK;
}

static long long rs_out_frames(const fmd_resampler_s* r, long long n_in) {
    if (r->fs_in == r->fs_out) return n_in;
    if (r->method == FMD_RESAMPLE_REFERENCE) return fmd::resample_ref_frames(r->fs_in, r->fs_out, n_in);
    const long long end = ((r->n_abs + n_in) * r->L + r->M - 1) / r->M;    // ceil: outputs n with floor(n M / L) < n_abs + n_in
    return end - r->o_abs;
}

template <typename OutT>
static int rs_process(fmd_resampler r, const float* d_in, long long in_stride, long long n_in, OutT* d_out, long long out_stride, long long* n_out,
                      hipStream_t s) {
    if (!r || !d_in || !d_out || !n_out) return FMD_ERR_ARG;
    if (n_in < 0 || n_in > r->max_in || in_stride < n_in) return rs_fail(r, FMD_ERR_SIZE, "n_in %lld outside [0, min(in_stride %lld, max_input_frames %lld)]", n_in, in_stride, r->max_in);
    const long long no = rs_out_frames(r, n_in);
    if (no > out_stride) return rs_fail(r, FMD_ERR_SIZE, "out_stride %lld < %lld output frames", out_stride, no);
    const fmd_resampler_s::Table* tab = nullptr;
    if (r->method == FMD_RESAMPLE_REFERENCE && r->fs_in != r->fs_out && no > 0) {
        auto it = r->tables.find(n_in);
        if (it == r->tables.end()) {
            fmd_resampler_s::Table t;
            t.n_out = (int)no;
            if (!fmd::resample_ref_table((int)n_in, (int)no, &t.host))
                return rs_fail(r, FMD_ERR_ARG, "the reference's index leaves the %lld-frame input before its %lld outputs are made (its span indexing would abort)", n_in, no);
            if (r->tables.size() >= kMaxTables) {
                if (!r->order.quiesce()) return rs_fail(r, FMD_ERR_DEVICE, "synchronise failed");
                rs_free_tables(r);
            }
            if (hipSetDevice(r->order.device()) != hipSuccess || hipMalloc(&t.dev, sizeof(int4) * (size_t)no) != hipSuccess ||
                hipMemcpy(t.dev, t.host.data(), sizeof(int4) * (size_t)no, hipMemcpyHostToDevice) != hipSuccess) {
                if (t.dev) (void)hipFree(t.dev);
                return rs_fail(r, FMD_ERR_DEVICE, "index table upload failed");
            }
            it = r->tables.emplace(n_in, std::move(t)).first;
        }
        tab = &it->second;
    }
    if (const char* e = r->order.begin(s)) return rs_fail(r, FMD_ERR_DEVICE, "%s", e);
    const unsigned gy = (unsigned)((r->C + kStations - 1) / kStations);
    const float2* in = reinterpret_cast<const float2*>(d_in);
    bool launched = false;
    if (r->fs_in == r->fs_out) {
        if (n_in > 0) {
            hipLaunchKernelGGL(k_resample_copy<OutT>, dim3((unsigned)((n_in + 255) / 256), gy), dim3(256), 0, s, in, in_stride, n_in, d_out, out_stride, r->C);
            launched = true;
        }
    } else if (r->method == FMD_RESAMPLE_REFERENCE) {
        if (no > 0) {
            hipLaunchKernelGGL(k_resample_ref<OutT>, dim3((unsigned)((no + 255) / 256), gy), dim3(256), 0, s, in, in_stride, (int)n_in, tab->dev, (int)no,
                               d_out, out_stride, r->C);
            launched = true;
        }
    } else if (n_in > 0) {
        const PolyDims d{r->L, r->M, r->T, r->C, r->tile, r->win, n_in, in_stride, no, out_stride, r->o_abs, r->n_abs};
        const unsigned gx = (unsigned)(no > 0 ? (no + r->tile - 1) / r->tile : 1);
        hipLaunchKernelGGL(k_resample_poly<OutT>, dim3(gx, gy), dim3(256), sizeof(float2) * (size_t)kStations * r->win, s, d, in, r->hist[r->cur],
                           r->hist[r->cur ^ 1], r->taps, d_out);
        launched = true;
        r->cur ^= 1;
    }
    if (launched && hipGetLastError() != hipSuccess) return rs_fail(r, FMD_ERR_DEVICE, "resampler launch failed");
    if (const char* e = r->order.end(s)) return rs_fail(r, FMD_ERR_DEVICE, "%s", e);
    if (r->method == FMD_RESAMPLE_POLYPHASE) { r->n_abs += n_in; r->o_abs += no; }
    *n_out = no;
    return FMD_OK;
}

extern "C" {

int fmd_resampler_design(int fs_in, int fs_out, int taps_per_phase, float* taps, int* L, int* M) {
    int l = 0, m = 0;
    if (!fmd::resample_poly_design(fs_in, fs_out, 8, nullptr, &l, &m)) return FMD_ERR_ARG;
    const int T = taps_per_phase > 0 ? taps_per_phase : default_taps(l, m);
    if (T % 4 != 0) return FMD_ERR_ARG;
    std::vector<float> h;
    if (!fmd::resample_poly_design(fs_in, fs_out, T, taps ? &h : nullptr, L, M)) return FMD_ERR_ARG;
    if (taps) std::memcpy(taps, h.data(), sizeof(float) * h.size());
    return FMD_OK;
}

int fmd_resampler_create(const fmd_resampler_config* cfg, fmd_resampler* out) {
    if (!cfg || !out || cfg->n_channels <= 0 || cfg->max_input_frames <= 0 || cfg->max_input_frames > (1 << 30) || cfg->fs_in <= 0 || cfg->fs_out <= 0 ||
        (cfg->method != FMD_RESAMPLE_REFERENCE && cfg->method != FMD_RESAMPLE_POLYPHASE))
        return rs_fail(nullptr, FMD_ERR_ARG, "bad resampler configuration");
    if (cfg->method == FMD_RESAMPLE_POLYPHASE && fmd_resampler_design(cfg->fs_in, cfg->fs_out, cfg->taps_per_phase, nullptr, nullptr, nullptr) != FMD_OK)
        return rs_fail(nullptr, FMD_ERR_ARG, "unsupported polyphase rates %d -> %d with %d taps per phase", cfg->fs_in, cfg->fs_out, cfg->taps_per_phase);
    if (fmd_device_count() <= 0) return rs_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return rs_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_resampler r = new fmd_resampler_s();
    r->C = cfg->n_channels; r->fs_in = cfg->fs_in; r->fs_out = cfg->fs_out; r->method = cfg->method; r->T_cfg = cfg->taps_per_phase;
    r->max_in = cfg->max_input_frames;
    bool ok = r->order.init(dev);
    if (ok && r->method == FMD_RESAMPLE_POLYPHASE) {
        {
            const int rc = rs_setup_poly(r);
            if (rc != FMD_OK) { std::string e = r->err; fmd_resampler_destroy(r); return rs_fail(nullptr, rc, "%s", e.c_str()); }
        }
    }
    if (!ok) { fmd_resampler_destroy(r); return rs_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed"); }
    *out = r;
    return FMD_OK;
}

int fmd_resampler_destroy(fmd_resampler r) {
    if (!r) return FMD_ERR_ARG;
    (void)r->order.quiesce();
    rs_free_tables(r);
    for (int i = 0; i < 2; i++) if (r->hist[i]) (void)hipFree(r->hist[i]);
    if (r->taps) (void)hipFree(r->taps);
    if (r->scratch) (void)hipFree(r->scratch);
    delete r;
    return FMD_OK;
}

int fmd_resampler_reset(fmd_resampler r, int channel) {
    if (!r || channel < -1 || channel >= r->C) return FMD_ERR_ARG;
    if (r->method != FMD_RESAMPLE_POLYPHASE) return FMD_OK;
    if (!r->order.quiesce()) return rs_fail(r, FMD_ERR_DEVICE, "synchronise failed");
    const size_t row = sizeof(float2) * (size_t)(r->T - 1);
    if (channel < 0) {
        for (int i = 0; i < 2; i++)
            if (hipMemset(r->hist[i], 0, row * (size_t)r->C) != hipSuccess) return rs_fail(r, FMD_ERR_DEVICE, "memset failed");
        r->n_abs = 0; r->o_abs = 0; r->cur = 0;
    } else if (hipMemset(reinterpret_cast<char*>(r->hist[r->cur]) + row * (size_t)channel, 0, row) != hipSuccess) {
        return rs_fail(r, FMD_ERR_DEVICE, "memset failed");
    }
    return FMD_OK;
}

int fmd_resampler_set_input_rate(fmd_resampler r, int fs_in) {
    if (!r || fs_in <= 0) return FMD_ERR_ARG;
    if (fs_in == r->fs_in) return 0;
    if (r->method == FMD_RESAMPLE_POLYPHASE && fmd_resampler_design(fs_in, r->fs_out, r->T_cfg, nullptr, nullptr, nullptr) != FMD_OK)
        return rs_fail(r, FMD_ERR_ARG, "unsupported polyphase rates %d -> %d", fs_in, r->fs_out);
    if (!r->order.quiesce()) return rs_fail(r, FMD_ERR_DEVICE, "synchronise failed");
    rs_free_tables(r);
    r->fs_in = fs_in;
    if (r->method == FMD_RESAMPLE_POLYPHASE) {
        const int rc = rs_setup_poly(r);
        if (rc != FMD_OK) return rc;
    }
    return 1;
}

int fmd_resampler_output_frames(fmd_resampler r, long long n_in, long long* n_out) {
    if (!r || !n_out || n_in < 0) return FMD_ERR_ARG;
    *n_out = rs_out_frames(r, n_in);
    return FMD_OK;
}

int fmd_resampler_process_f32_dev(fmd_resampler r, const float* d_in, long long in_stride, long long n_in, float* d_out, long long out_stride,
                                  long long* n_out, void* stream) {
    return rs_process(r, d_in, in_stride, n_in, reinterpret_cast<float2*>(d_out), out_stride, n_out, static_cast<hipStream_t>(stream));
}

int fmd_resampler_process_pcm16_dev(fmd_resampler r, const float* d_in, long long in_stride, long long n_in, int16_t* d_out, long long out_stride,
                                    long long* n_out, void* stream) {
    return rs_process(r, d_in, in_stride, n_in, reinterpret_cast<short2*>(d_out), out_stride, n_out, static_cast<hipStream_t>(stream));
}

int fmd_resampler_process_f32_host(fmd_resampler r, const float* d_in, long long in_stride, long long n_in, float* out, long long out_stride,
                                   long long* n_out, void* stream) {
    if (!r || !out || !n_out) return FMD_ERR_ARG;
    long long no = 0;
    fmd_resampler_output_frames(r, n_in < 0 ? 0 : n_in, &no);
    if (no > out_stride) return rs_fail(r, FMD_ERR_SIZE, "out_stride %lld < %lld output frames", out_stride, no);
    const size_t need = (size_t)r->C * (size_t)(no > 0 ? no : 1);
    if (need > r->scratch_frames) {
        if (!r->order.quiesce()) return rs_fail(r, FMD_ERR_DEVICE, "synchronise failed");
        if (r->scratch) (void)hipFree(r->scratch);
        r->scratch = nullptr; r->scratch_frames = 0;
        if (hipMalloc(&r->scratch, sizeof(float2) * need) != hipSuccess) return rs_fail(r, FMD_ERR_DEVICE, "scratch allocation failed");
        r->scratch_frames = need;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = rs_process(r, d_in, in_stride, n_in, r->scratch, no > 0 ? no : 1, n_out, s);
    if (rc != FMD_OK) return rc;
    if (*n_out > 0 && hipMemcpy2DAsync(out, sizeof(float2) * (size_t)out_stride, r->scratch, sizeof(float2) * (size_t)*n_out, sizeof(float2) * (size_t)*n_out,
                                       (size_t)r->C, hipMemcpyDeviceToHost, s) != hipSuccess)
        return rs_fail(r, FMD_ERR_DEVICE, "copy to the host failed");
    if (hipStreamSynchronize(s) != hipSuccess) return rs_fail(r, FMD_ERR_DEVICE, "synchronise failed");
    return FMD_OK;
}

const char* fmd_resampler_last_error(fmd_resampler r) { return r ? r->err.c_str() : g_rs_error.c_str(); }

}  // extern "C"
