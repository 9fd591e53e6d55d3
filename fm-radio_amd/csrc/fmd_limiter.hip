// Look-ahead peak limiter, device side (include/fmdemod.h, "Look-ahead peak limiter").
//
// NOT in the reference.  Per station: a gain, a linked sample peak, the gain the ceiling requires in Q30, and then three exact integer
// scans: a sliding minimum over W = D + 1 frames (the look-ahead), a slope-limited prefix minimum (the release) and a sliding sum over
// W frames (the attack).  Integers make every scan associative, so the tiling below cannot show in the bits.
//
// One workgroup of kT threads a station.  It walks the call's frames in tiles of kTile.  A tile is worked on as an "extended" array in
// LDS: positions 0 ... D - 1 hold what the station carries (the last D values of u, rq and eq), positions D ... D + len - 1 the tile's
// frames, so that every window of the tile lies inside the array.  Loads are 16 bytes a lane (two frames), coalesced; u, p and rq are
// made at the load.  The sliding minimum is by doubling in LDS, floor(log2 W) passes and one combine.  For the two prefix scans every
// thread owns kItems consecutive positions of the extended array: a serial scan in registers, __shfl_up steps inside the wavefront, one
// LDS hop across the wavefronts.  The release is the prefix minimum of mq[j] - j * step in int64, then + j * step and the carry-in term;
// the sliding sum is a difference of the exact uint64 prefix sum.  The store is 16 bytes a lane again.  After a tile the last D
// positions move to the front; the last tile hands them to the station's state in device memory.  Flush is the same walk over D frames
// of silence.  Counters are reduced in registers, by wavefront and by one LDS hop, once a call.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fmd_limiter_design.h"
#include "fmd_side.h"
#include "fmdemod.h"
#include "fmdemod_limiter_debug.h"

namespace {

// the launch geometry, in one place: nothing in the arithmetic depends on it
constexpr int kT = 256;                      // threads per workgroup: four wavefronts
constexpr int kWaves = kT / 64;
constexpr int kItems = 5;                    // positions of the extended array that a thread owns in the scans
constexpr int kExt = kT * kItems;            // the extended array: 1280 positions
constexpr int kTile = 1024;                  // frames per tile: two 16-byte loads a lane
constexpr int kHist = 256;                   // the carried positions: D <= 255
constexpr uint32_t kOne = fmd::kLimiterOne;
static_assert(kHist + kTile <= kExt && fmd::kLimiterMaxD < kHist && kHist <= kT && kTile % (2 * kT) == 0, "k_limiter's tile layout");

static_assert(sizeof(fmd_limiter_status) == 64 && offsetof(fmd_limiter_status, limited) == 8 && offsetof(fmd_limiter_status, clamped) == 16 &&
              offsetof(fmd_limiter_status, nonfinite) == 32 && offsetof(fmd_limiter_status, min_gain) == 40 && offsetof(fmd_limiter_status, gain) == 44 &&
              offsetof(fmd_limiter_status, eq) == 48 && offsetof(fmd_limiter_status, reserved) == 52,
              "fmd_limiter_status layout");

typedef float lim_f4 __attribute__((ext_vector_type(4), aligned(8)));        // a station's rows are aligned to a frame only
typedef float lim_f2 __attribute__((ext_vector_type(2)));

// what a station carries beside its record: the last D values, oldest first, in rows of D
struct LimState {
    float2* u;       // [C][D]
    uint32_t* rq;    // [C][D]
    uint32_t* eq;    // [C][D]
};

struct OpMin { __device__ long long operator()(long long a, long long b) const { return a < b ? a : b; } };
struct OpAdd { __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; } };

// the exclusive scan, over the workgroup's threads in order, of one value a thread; s_w [kWaves] is free again on return
template <typename V, typename Op>
__device__ __forceinline__ V lim_scan_excl(V v, V identity, Op op, V* s_w, int lane, int wave) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const V t = __shfl_up(v, o);
        if (lane >= o) v = op(t, v);
    }
    V exc = __shfl_up(v, 1);
    if (lane == 0) exc = identity;
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    V pre = identity;
    for (int w = 0; w < wave; w++) pre = op(pre, s_w[w]);
    __syncthreads();
    return op(pre, exc);
}

// one rail: u = x * gain, or +0 and a count where that is not finite
__device__ __forceinline__ float lim_u(float x, float gain, unsigned& nonf) {
    const float u = x * gain;
    if (!(fabsf(u) <= 3.402823466e38f)) { nonf++; return 0.0f; }
    return u;
}

// the gain the ceiling requires of a frame, Q30
__device__ __forceinline__ uint32_t lim_rq(float ul, float ur, float T) {
    const float p = fmaxf(fabsf(ul), fabsf(ur));
    if (p <= T) return kOne;
    return (uint32_t)((T / p) * 1073741824.0f);
}

// station c: n frames of `in` (kFlush: D frames of silence) through the limiter, written at `out`
template <bool kFlush>
__device__ __forceinline__ void lim_run(const float2* __restrict__ in, int n, int c, int D, uint32_t step, float T, fmd_limiter_status* __restrict__ status,
                                        const LimState st, float2* __restrict__ out, float* __restrict__ gr) {
    __shared__ float2 s_u[kExt];
    __shared__ uint32_t s_rq[kExt];
    __shared__ uint32_t s_eq[kExt];
    __shared__ unsigned long long s_ps[kExt];
    uint32_t* s_a = reinterpret_cast<uint32_t*>(s_ps);                       // the doubling's array is done with before the prefix sums are stored
    __shared__ long long s_wmin[kWaves];
    __shared__ unsigned long long s_wsum[kWaves];
    __shared__ uint32_t s_carry;
    __shared__ unsigned s_cnt[kWaves][4];
    __shared__ float s_gmin[kWaves];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = D + 1;
    fmd_limiter_status* stp = status + c;
    if (n == 0) {                                                            // (uniform) nothing of the station's signal state moves
        if (tid == 0 && gr) gr[c] = 1.0f;
        return;
    }
    const float gain = stp->gain;
    const float wf = (float)((unsigned long long)W << 30);                   // W * 2^30: exact in fp32 (W <= 256)
    const unsigned long long full = (unsigned long long)W << 30;
    uint32_t eq_in = stp->eq;
    const size_t hrow = (size_t)c * (size_t)D;
    if (tid < D) {
        s_u[tid] = st.u[hrow + tid];
        s_rq[tid] = st.rq[hrow + tid];
        s_eq[tid] = st.eq[hrow + tid];
    }
    unsigned nonf = 0u, limited = 0u, clampl = 0u, clampr = 0u;              // this thread's share of the call's counts
    float gmin = 1.0f;

    for (int t0 = 0; t0 < n; t0 += kTile) {
        const int len = n - t0 < kTile ? n - t0 : kTile;
        const int L = D + len;                                               // the extended array's length (<= kExt - 1)
        // ---- the tile's frames: u and rq behind the carried positions
#pragma unroll
        for (int k = 0; k < kTile / (2 * kT); k++) {
            const int t = k * 2 * kT + 2 * tid;
            if (t >= len) continue;
            lim_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (!kFlush) {
                const float2* p = in + (size_t)t0 + (size_t)t;
                if (t + 1 < len) v = __builtin_nontemporal_load(reinterpret_cast<const lim_f4*>(p));
                else {
                    const lim_f2 a = __builtin_nontemporal_load(reinterpret_cast<const lim_f2*>(p));
                    v.x = a.x; v.y = a.y;
                }
            }
            const float ul0 = lim_u(v.x, gain, nonf), ur0 = lim_u(v.y, gain, nonf);
            s_u[D + t] = make_float2(ul0, ur0);
            s_rq[D + t] = lim_rq(ul0, ur0, T);
            if (t + 1 < len) {
                const float ul1 = lim_u(v.z, gain, nonf), ur1 = lim_u(v.w, gain, nonf);
                s_u[D + t + 1] = make_float2(ul1, ur1);
                s_rq[D + t + 1] = lim_rq(ul1, ur1, T);
            }
        }
        __syncthreads();
        // ---- the look-ahead: a[i] = min(rq[i - s + 1 ... i]) by doubling, s the largest power of two <= W.  A position below s - 1
        // has a shorter window; none of those is read below (i >= D and i - (W - s) >= s - 1)
        const int i0 = tid * kItems;
#pragma unroll
        for (int q = 0; q < kItems; q++)
            if (i0 + q < L) s_a[i0 + q] = s_rq[i0 + q];
        __syncthreads();
        int s = 1;
        for (; 2 * s <= W; s <<= 1) {                                        // (uniform)
            uint32_t m[kItems];
#pragma unroll
            for (int q = 0; q < kItems; q++) {
                const int i = i0 + q;
                m[q] = kOne;
                if (i < L) {
                    m[q] = s_a[i];
                    if (i >= s) { const uint32_t b = s_a[i - s]; m[q] = b < m[q] ? b : m[q]; }
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kItems; q++)
                if (i0 + q < L) s_a[i0 + q] = m[q];
            __syncthreads();
        }
        // ---- the release: eq[i] = min(eq_in + (i - D + 1) * step, min over D <= j <= i of (mq[j] - j * step) + i * step)
        long long v[kItems];
        long long run = INT64_MAX;
#pragma unroll
        for (int q = 0; q < kItems; q++) {
            const int i = i0 + q;
            long long x = INT64_MAX;
            if (i >= D && i < L) {
                const uint32_t a = s_a[i], b = s_a[i - (W - s)];
                x = (long long)(a < b ? a : b) - (long long)i * (long long)step;
            }
            run = x < run ? x : run;
            v[q] = run;                                                      // the thread's own inclusive prefix
        }
        const long long pre = lim_scan_excl<long long>(run, INT64_MAX, OpMin(), s_wmin, lane, wave);
        unsigned long long e[kItems];
        unsigned long long sum = 0ull;
#pragma unroll
        for (int q = 0; q < kItems; q++) {
            const int i = i0 + q;
            unsigned long long x = 0ull;
            if (i < D) x = s_eq[i];
            else if (i < L) {
                const long long m = v[q] < pre ? v[q] : pre;                 // (finite: position i itself is under it)
                const long long a = m + (long long)i * (long long)step;
                const long long b = (long long)eq_in + (long long)(i - D + 1) * (long long)step;
                x = (unsigned long long)(a < b ? a : b);
                s_eq[i] = (uint32_t)x;
                if (i == L - 1) s_carry = (uint32_t)x;
            }
            sum += x;
            e[q] = sum;
        }
        // ---- the attack: the inclusive prefix sum of eq over the extended array
        const unsigned long long psum = lim_scan_excl<unsigned long long>(sum, 0ull, OpAdd(), s_wsum, lane, wave);
#pragma unroll
        for (int q = 0; q < kItems; q++)
            if (i0 + q < L) s_ps[i0 + q] = psum + e[q];
        __syncthreads();
        // ---- the output: frame t of the tile is position D + t; its window's sum is ps[D + t] - ps[t - 1], its delayed frame u[t]
#pragma unroll
        for (int k = 0; k < kTile / (2 * kT); k++) {
            const int t = k * 2 * kT + 2 * tid;
            if (t >= len) continue;
            float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int f = 0; f < 2; f++) {
                const int tt = t + f;
                if (tt >= len) break;
                const unsigned long long S = s_ps[D + tt] - (tt > 0 ? s_ps[tt - 1] : 0ull);
                const float g = (float)S / wf;
                if (S < full) limited++;
                gmin = g < gmin ? g : gmin;
                const float2 u = s_u[tt];
                float yl = u.x * g, yr = u.y * g;
                if (yl > T) { yl = T; clampl++; } else if (yl < -T) { yl = -T; clampl++; }
                if (yr > T) { yr = T; clampr++; } else if (yr < -T) { yr = -T; clampr++; }
                y[2 * f] = yl; y[2 * f + 1] = yr;
            }
            float2* p = out + (size_t)t0 + (size_t)t;
            if (t + 1 < len) {
                const lim_f4 o = {y[0], y[1], y[2], y[3]};
                *reinterpret_cast<lim_f4*>(p) = o;
            } else {
                *p = make_float2(y[0], y[1]);
            }
        }
        // ---- the last D positions become the carried ones (the ranges overlap where len < D: through registers)
        float2 hu = make_float2(0.0f, 0.0f);
        uint32_t hr = kOne, he = kOne;
        if (tid < D) { hu = s_u[len + tid]; hr = s_rq[len + tid]; he = s_eq[len + tid]; }
        eq_in = s_carry;
        __syncthreads();
        if (tid < D) { s_u[tid] = hu; s_rq[tid] = hr; s_eq[tid] = he; }
    }

    // ---- the station's state and counts
    if (tid < D) {
        if (kFlush) {
            st.u[hrow + tid] = make_float2(0.0f, 0.0f); st.rq[hrow + tid] = kOne; st.eq[hrow + tid] = kOne;
        } else {
            st.u[hrow + tid] = s_u[tid]; st.rq[hrow + tid] = s_rq[tid]; st.eq[hrow + tid] = s_eq[tid];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nonf += __shfl_down(nonf, o); limited += __shfl_down(limited, o);
        clampl += __shfl_down(clampl, o); clampr += __shfl_down(clampr, o);
        const float g2 = __shfl_down(gmin, o);
        gmin = g2 < gmin ? g2 : gmin;
    }
    if (lane == 0) {
        s_cnt[wave][0] = nonf; s_cnt[wave][1] = limited; s_cnt[wave][2] = clampl; s_cnt[wave][3] = clampr;
        s_gmin[wave] = gmin;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned tot[4] = {0u, 0u, 0u, 0u};
        float g = 1.0f;
        for (int w = 0; w < kWaves; w++) {
            for (int k = 0; k < 4; k++) tot[k] += s_cnt[w][k];
            g = s_gmin[w] < g ? s_gmin[w] : g;
        }
        if (!kFlush) stp->frames += (unsigned long long)n;
        stp->nonfinite += tot[0];
        stp->limited += tot[1];
        stp->clamped[0] += tot[2];
        stp->clamped[1] += tot[3];
        const float old = stp->min_gain;
        stp->min_gain = g < old ? g : old;
        stp->eq = kFlush ? kOne : eq_in;
        if (gr) gr[c] = g;
    }
}

// in [C][in_stride] frames (L, R) -> out [C][out_stride]; status [C]; gr [C] or null
__global__ __launch_bounds__(kT) void k_limiter(const float2* __restrict__ in, long long in_stride, int n, const uint8_t* __restrict__ active, int D, uint32_t step,
                                                float T, fmd_limiter_status* __restrict__ status, LimState st, float2* __restrict__ out, long long out_stride,
                                                float* __restrict__ gr) {
    const int c = blockIdx.x;
    if (active && active[c] == 0) return;                                    // (uniform) a skipped station
    lim_run<false>(in + (size_t)c * (size_t)in_stride, n, c, D, step, T, status, st, out + (size_t)c * (size_t)out_stride, gr);
}

// stations c0 ... c0 + cn - 1: the D frames that D frames of silence push out; then the signal state of a reset
__global__ __launch_bounds__(kT) void k_limiter_flush(int c0, int D, uint32_t step, float T, fmd_limiter_status* __restrict__ status, LimState st,
                                                      float2* __restrict__ out, long long out_stride, int* __restrict__ nout) {
    const int c = c0 + blockIdx.x;
    lim_run<true>(nullptr, D, c, D, step, T, status, st, out + (size_t)c * (size_t)out_stride, nullptr);
    if (threadIdx.x == 0) {
        if (D == 0) status[c].eq = kOne;                                     // (no frame went through: the release state alone)
        if (nout) nout[c] = D;
    }
}

// stations c0 ... c0 + cn - 1 as after create, the gain kept
__global__ __launch_bounds__(kT) void k_limiter_reset(int c0, int D, fmd_limiter_status* __restrict__ status, LimState st) {
    const int c = c0 + blockIdx.x, tid = threadIdx.x;
    if (tid < D) {
        const size_t i = (size_t)c * (size_t)D + tid;
        st.u[i] = make_float2(0.0f, 0.0f); st.rq[i] = kOne; st.eq[i] = kOne;
    }
    if (tid == 0) {
        fmd_limiter_status r = {};
        r.gain = status[c].gain;
        r.min_gain = 1.0f;
        r.eq = kOne;
        status[c] = r;
    }
}

__global__ __launch_bounds__(kT) void k_limiter_set_gain(int c0, int cn, float gain, fmd_limiter_status* __restrict__ status) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < cn) status[c0 + i].gain = gain;
}

}  // namespace

struct fmd_limiter_s {
    int C = 0, D = 0;
    uint32_t step = 0;
    float T = 0.0f;
    long long max_in = 0;
    fmd_limiter_status* d_status = nullptr;  // [C]
    LimState st{nullptr, nullptr, nullptr};  // [C][max(D, 1)] each
    std::vector<float> gain;                 // [C]: as set
    fmd::CallOrder order;                    // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int lim_fail(fmd_limiter l, int code, const char* fmt, A... args) { return fmd::fail(l ? l->err : fmd::limiter_global_error(), code, fmt, args...); }

static int lim_set_gain(fmd_limiter l, int c0, int cn, float gain) {
    hipLaunchKernelGGL(k_limiter_set_gain, dim3((unsigned)((cn + kT - 1) / kT)), dim3(kT), 0, nullptr, c0, cn, gain, l->d_status);
    if (const char* m = fmd::control_end("k_limiter_set_gain launch failed")) return lim_fail(l, FMD_ERR_DEVICE, "%s", m);
    for (int c = c0; c < c0 + cn; c++) l->gain[(size_t)c] = gain;
    return FMD_OK;
}

extern "C" {

int fmd_limiter_create(const fmd_limiter_config* cfg, fmd_limiter* out) {
    if (!cfg || !out) return lim_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->n_channels <= 0 || cfg->max_input_frames <= 0 || cfg->max_input_frames > (1LL << 30))
        return lim_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_frames %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_frames);
    fmd_limiter_design_t d;
    if (fmd_limiter_design(cfg->fs, cfg->lookahead_ms, cfg->release_ms, cfg->ceiling_db, &d) != FMD_OK) return FMD_ERR_ARG;   // (the message is the design's)
    if (fmd_device_count() <= 0) return lim_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return lim_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_limiter l = new fmd_limiter_s();
    l->C = cfg->n_channels; l->D = d.lookahead_frames; l->step = d.step; l->T = d.ceiling; l->max_in = cfg->max_input_frames;
    l->gain.assign((size_t)l->C, 1.0f);
    const size_t C = (size_t)l->C, rows = C * (size_t)(l->D > 0 ? l->D : 1);
    bool ok = l->order.init(dev);
    ok = ok && hipMalloc(&l->d_status, sizeof(fmd_limiter_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&l->st.u, sizeof(float2) * rows) == hipSuccess;
    ok = ok && hipMalloc(&l->st.rq, sizeof(uint32_t) * rows) == hipSuccess;
    ok = ok && hipMalloc(&l->st.eq, sizeof(uint32_t) * rows) == hipSuccess;
    if (!ok || lim_set_gain(l, 0, l->C, 1.0f) != FMD_OK || fmd_limiter_reset(l, -1) != FMD_OK) {
        fmd_limiter_destroy(l);
        return lim_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed");
    }
    *out = l;
    return FMD_OK;
}

int fmd_limiter_destroy(fmd_limiter l) {
    if (!l) return FMD_ERR_ARG;
    (void)l->order.quiesce();
    for (void* p : {(void*)l->d_status, (void*)l->st.u, (void*)l->st.rq, (void*)l->st.eq})
        if (p) (void)hipFree(p);
    delete l;
    return FMD_OK;
}

int fmd_limiter_reset(fmd_limiter l, int channel) {
    if (!l) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, l->C, &c0, &cn)) return lim_fail(l, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, l->C);
    if (!l->order.quiesce()) return lim_fail(l, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_limiter_reset, dim3((unsigned)cn), dim3(kT), 0, nullptr, c0, l->D, l->d_status, l->st);
    if (const char* m = fmd::control_end("k_limiter_reset launch failed")) return lim_fail(l, FMD_ERR_DEVICE, "%s", m);
    return FMD_OK;
}

int fmd_limiter_set_gain(fmd_limiter l, int channel, float gain) {
    if (!l) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, l->C, &c0, &cn)) return lim_fail(l, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, l->C);
    if (!(gain >= 0.0f) || !(gain <= 3.402823466e38f)) return lim_fail(l, FMD_ERR_ARG, "the gain is negative or not finite");
    if (!l->order.quiesce()) return lim_fail(l, FMD_ERR_DEVICE, "synchronise failed");
    return lim_set_gain(l, c0, cn, gain);
}

int fmd_limiter_get_gain(fmd_limiter l, int channel, float* gain) {
    if (!l) return FMD_ERR_ARG;
    if (!gain || channel < 0 || channel >= l->C) return lim_fail(l, FMD_ERR_ARG, "null output, or channel %d outside [0, %d)", channel, l->C);
    *gain = l->gain[(size_t)channel];
    return FMD_OK;
}

int fmd_limiter_process_f32_dev(fmd_limiter l, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, float* d_out, long long out_stride,
                                float* d_gr, void* stream) {
    if (!l) return FMD_ERR_ARG;
    if (fmd::limiter_check_call(l->C, l->max_in, d_in, in_stride, n, d_out, out_stride, &l->err) != FMD_OK) return FMD_ERR_ARG;
    if (n == 0 && !d_gr) return FMD_OK;                                      // nothing of any station changes and there is no gain to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* m = l->order.begin(s)) return lim_fail(l, FMD_ERR_DEVICE, "%s", m);
    hipLaunchKernelGGL(k_limiter, dim3((unsigned)l->C), dim3(kT), 0, s, reinterpret_cast<const float2*>(d_in), in_stride, (int)n, d_active, l->D, l->step, l->T,
                       l->d_status, l->st, reinterpret_cast<float2*>(d_out), out_stride, d_gr);
    if (hipGetLastError() != hipSuccess) return lim_fail(l, FMD_ERR_DEVICE, "k_limiter launch failed");
    if (const char* m = l->order.end(s)) return lim_fail(l, FMD_ERR_DEVICE, "%s", m);
    return FMD_OK;
}

int fmd_limiter_flush(fmd_limiter l, int channel, float* d_out, long long out_stride, int* d_nout, void* stream) {
    if (!l) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, l->C, &c0, &cn)) return lim_fail(l, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, l->C);
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 8 != 0) return lim_fail(l, FMD_ERR_ARG, "null output, or output not aligned to 8 bytes");
    if (out_stride < l->D) return lim_fail(l, FMD_ERR_ARG, "out_stride %lld is below the %d frames a flush writes", out_stride, l->D);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const char* m = l->order.begin(s)) return lim_fail(l, FMD_ERR_DEVICE, "%s", m);
    hipLaunchKernelGGL(k_limiter_flush, dim3((unsigned)cn), dim3(kT), 0, s, c0, l->D, l->step, l->T, l->d_status, l->st, reinterpret_cast<float2*>(d_out), out_stride,
                       d_nout);
    if (hipGetLastError() != hipSuccess) return lim_fail(l, FMD_ERR_DEVICE, "k_limiter_flush launch failed");
    if (const char* m = l->order.end(s)) return lim_fail(l, FMD_ERR_DEVICE, "%s", m);
    return FMD_OK;
}

int fmd_limiter_get_status(fmd_limiter l, fmd_limiter_status* out) {
    if (!l || !out) return lim_fail(l, FMD_ERR_ARG, "null limiter or output");
    if (!l->order.quiesce()) return lim_fail(l, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, l->d_status, sizeof(fmd_limiter_status) * (size_t)l->C, hipMemcpyDeviceToHost) != hipSuccess) return lim_fail(l, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_limiter_status_dev(fmd_limiter l, const fmd_limiter_status** d_status) {
    if (!l || !d_status) return lim_fail(l, FMD_ERR_ARG, "null limiter or output");
    *d_status = l->d_status;
    return FMD_OK;
}

const char* fmd_limiter_last_error(fmd_limiter l) { return l ? l->err.c_str() : fmd::limiter_global_error().c_str(); }

int fmd_limiter_debug_set_frames(fmd_limiter l, int channel, unsigned long long frames) {
    if (!l) return FMD_ERR_ARG;
    if (channel < 0 || channel >= l->C) return lim_fail(l, FMD_ERR_ARG, "channel %d outside [0, %d)", channel, l->C);
    if (!l->order.quiesce()) return lim_fail(l, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(&l->d_status[channel].frames, &frames, sizeof(frames), hipMemcpyHostToDevice) != hipSuccess) return lim_fail(l, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

}  // extern "C"
