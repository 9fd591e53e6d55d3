// EAS SAME decoder, device side (include/fmdemod.h, "EAS SAME decoder").
//
// NOT in the reference.  Per station the mid signal m = L + R of the station audio [C][in_stride][2] f32 that the mixer and the monitors
// read, read in place, is correlated against the mark (2083.33 Hz) and the space tone (1562.5 Hz) in ticks of an eighth of a bit; at a
// tick's end the two tones' energies over the last eight ticks are compared, and the one bit that comes of it drives an integer bit clock
// and a byte framer that collects `ZCZC...` and `NNNN` messages into the station's record.
//
// One kernel per call, k_same: one wavefront per station over rows of 64 consecutive ticks, the open tick first.  A row's frames (at most
// 739: 64 ticks of 11.52 frames at 48 kHz) are loaded by the whole wavefront with coalesced 8-byte non-temporal loads into LDS; lane l
// then owns tick l of the row and adds its frames in ascending order, with two 16-byte gathers per frame from the handle's table in
// global memory (at most 922 KB, shared by every station: it stays in L2) whose indices move by an add and a conditional subtract.  The
// lanes' four sums go to LDS behind the seven ticks before the row, so that lane l reads its window as eight consecutive entries per sum
// (component-major: no bank conflicts).  The row's decisions are one 64-bit ballot.  The clock and the framer are walked over that mask
// wave-uniformly -- their state is read through readfirstlane, so it lives in scalar registers -- and lane 0 alone stores, with ordinary
// vector stores: the message bytes as they arrive, the ring entry when a message is accepted, the record at the call's end.  No atomics,
// no scratch.
//
// Denormals: fp64 and fp32 denormals are kept (hipcc's default mode; this file is NOT built with -fgpu-flush-denormals-to-zero).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fmd_same_design.h"
#include "fmd_side.h"
#include "fmdemod.h"

using fmd::kSameHist;
using fmd::kSameTickPeriod;

namespace {

constexpr int kT = 64;                       // threads per workgroup: one wavefront, one station, a row of 64 ticks
constexpr int kRowFrames = 768;              // a row's frames: off(r + 64) - off(r) <= ceil(64 * 11.52) = 738, + 1 for the two roundings
constexpr int kSumStride = kSameHist + kT + 1;
constexpr unsigned kZCZC = 0x435A435Au, kNNNN = 0x4E4E4E4Eu;   // the first four bytes, little-endian
static_assert(kSameHist == 7 && kSameTickPeriod == 12500, "k_same's window and tick grid");

static_assert(sizeof(fmd_same_message) == 280 && offsetof(fmd_same_message, len) == 8 && offsetof(fmd_same_message, kind) == 10 &&
              offsetof(fmd_same_message, bytes) == 12, "fmd_same_message layout");
static_assert(sizeof(fmd_same_status) == 2856 && offsetof(fmd_same_status, ticks) == 8 && offsetof(fmd_same_status, bits) == 16 &&
              offsetof(fmd_same_status, syncs) == 24 && offsetof(fmd_same_status, accepted) == 32 && offsetof(fmd_same_status, rejected) == 40 &&
              offsetof(fmd_same_status, sync_tick) == 48 && offsetof(fmd_same_status, last_accept_tick) == 56 && offsetof(fmd_same_status, open) == 64 &&
              offsetof(fmd_same_status, hist) == 96 && offsetof(fmd_same_status, ph) == 320 && offsetof(fmd_same_status, sh) == 324 &&
              offsetof(fmd_same_status, nbit) == 328 && offsetof(fmd_same_status, msg_len) == 332 && offsetof(fmd_same_status, run) == 336 &&
              offsetof(fmd_same_status, synced) == 340 && offsetof(fmd_same_status, prev_s) == 341 && offsetof(fmd_same_status, flags) == 342 &&
              offsetof(fmd_same_status, ok) == 343 && offsetof(fmd_same_status, msg) == 344 && offsetof(fmd_same_status, ring) == 616, "fmd_same_status layout");
static_assert(sizeof(fmd_same_params) == 16, "fmd_same_params layout");

typedef float sm_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float2 sm_load1(const float2* p) {
    const sm_f2 v = __builtin_nontemporal_load(reinterpret_cast<const sm_f2*>(p));
    return make_float2(v.x, v.y);
}

// a + b mod P for a, b < P
__device__ __forceinline__ unsigned sm_step(unsigned a, unsigned b, unsigned P) {
    const unsigned s = a + b;
    return s >= P ? s - P : s;
}

__device__ __forceinline__ unsigned sm_uni(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long sm_uni64(unsigned long long v) {
    return ((unsigned long long)sm_uni((unsigned)(v >> 32)) << 32) | (unsigned long long)sm_uni((unsigned)v);
}

// in [C][in_stride] frames (L, R); tab [P] (cos, sin); prm [C]; status [C]; out_flags, out_ok [C] or null
__global__ __launch_bounds__(kT) void k_same(const float2* __restrict__ in, long long in_stride, long long n, const uint8_t* __restrict__ active, int fs, int P,
                                             int mark_step, int space_step, const double2* __restrict__ tab, const fmd_same_params* __restrict__ prm,
                                             fmd_same_status* __restrict__ status, uint8_t* __restrict__ out_flags, uint8_t* __restrict__ out_ok) {
    __shared__ float2 fr[kRowFrames];
    __shared__ double sums[4][kSumStride];                                   // per sum: the seven ticks before the row, then the row's 64
    const int c = blockIdx.x, lane = threadIdx.x;
    if (active && active[c] == 0) return;                                    // (uniform over the wavefront)
    fmd_same_status* st = status + c;
    const float2* base = in + (size_t)c * (size_t)in_stride;
    const unsigned uP = (unsigned)P, ms = (unsigned)mark_step, ss = (unsigned)space_step;
    const unsigned long long fs3 = 3ull * (unsigned long long)fs;

    // the parameters in force and the serial state, wave-uniform
    const unsigned pull = sm_uni((unsigned)prm[c].pull), hold = sm_uni(prm[c].hold_ticks), alarm_mask = sm_uni(prm[c].alarm_mask);
    const unsigned long long F0 = sm_uni64(st->frames), T0 = sm_uni64(st->ticks);
    unsigned long long bits = sm_uni64(st->bits), syncs = sm_uni64(st->syncs), accepted = sm_uni64(st->accepted), rejected = sm_uni64(st->rejected);
    unsigned long long sync_tick = sm_uni64(st->sync_tick), last_accept = sm_uni64(st->last_accept_tick);
    unsigned ph = sm_uni(st->ph), sh = sm_uni(st->sh), nbit = sm_uni(st->nbit), msg_len = sm_uni(st->msg_len);
    unsigned synced = sm_uni(st->synced), prev_s = sm_uni(st->prev_s), flags = sm_uni(st->flags), run = sm_uni(st->run);
    unsigned head = sm_uni(*reinterpret_cast<const unsigned*>(st->msg));     // the message's first four bytes (offset 344: aligned)
    if (msg_len < 4u) head &= (1u << (8u * msg_len)) - 1u;

    // tick T0 + j of the call is tick Tr + j of the period that starts org frames into the call (org <= 0)
    const unsigned Tr = (unsigned)(T0 % (unsigned long long)kSameTickPeriod);
    const long long org = (long long)((T0 / (unsigned long long)kSameTickPeriod) * fs3 - F0);
    const unsigned fm = (unsigned)(F0 % (unsigned long long)uP);             // the first frame's number mod P
    // the call's frame at which tick r of that period starts (r below 2^31: n <= 2^30 frames are fewer ticks)
    auto off = [&](unsigned r) -> long long {
        const unsigned q = r / (unsigned)kSameTickPeriod, r2 = r - q * (unsigned)kSameTickPeriod;
        return org + (long long)((unsigned long long)q * fs3) + (long long)((r2 * (unsigned)fs3 + 12499u) / 12500u);
    };
    auto clampn = [&](long long v) -> long long { return v < 0 ? 0 : (v > n ? n : v); };

    if (lane < kSameHist) {
#pragma unroll
        for (int k = 0; k < 4; k++) sums[k][lane] = st->hist[lane][k];
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) acc[k] = st->open[k];                    // the open tick goes on from its sums
    }
    double open[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned j0 = 0, done = 0;                                               // the row's first tick, counted from T0, and the ticks completed
    for (;;) {
        const unsigned r = Tr + j0 + (unsigned)lane;
        const long long e = off(r + 1u);
        const long long a = clampn(off(r)), b = clampn(e);
        const bool complete = e <= n;
        const long long rowA = clampn(off(Tr + j0)), rowB = clampn(off(Tr + j0 + (unsigned)kT));   // (uniform)
        __syncthreads();                                                     // the row before has been read
        for (long long i = rowA + lane; i < rowB; i += kT) fr[(int)(i - rowA)] = sm_load1(base + i);
        __syncthreads();
        if (a < b) {
            unsigned im = (unsigned)(((unsigned long long)fm + (unsigned long long)a) % (unsigned long long)uP), is = im;
            im = (im * ms) % uP;                                             // (below 2^32: P <= 57600)
            is = (is * ss) % uP;
            for (int i = (int)(a - rowA); i < (int)(b - rowA); i++) {
                const float2 v = fr[i];
                const double m = (double)v.x + (double)v.y;
                const double2 t1 = tab[im], t0 = tab[is];
                acc[0] = fma(m, t1.x, acc[0]);
                acc[1] = fma(m, t1.y, acc[1]);
                acc[2] = fma(m, t0.x, acc[2]);
                acc[3] = fma(m, t0.y, acc[3]);
                im = sm_step(im, ms, uP);
                is = sm_step(is, ss, uP);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) sums[k][kSameHist + lane] = acc[k];
        __syncthreads();
        double w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            w[k] = 0.0;
#pragma unroll
            for (int d = 0; d <= kSameHist; d++) w[k] += sums[k][lane + d];  // ticks k - 7 ... k, in that order
        }
        const double e1 = fma(w[0], w[0], w[1] * w[1]), e0 = fma(w[2], w[2], w[3] * w[3]);
        const unsigned long long mask = __ballot(complete && e1 > e0);
        const int nc = __popcll(__ballot(complete));                         // the row's completed ticks: its first nc

        for (int j = 0; j < nc; j++) {                                       // (everything here is wave-uniform)
            const unsigned long long k = T0 + (unsigned long long)j0 + (unsigned long long)j;
            const unsigned s = (unsigned)((mask >> j) & 1ull);
            if (s != prev_s) {
                // the run that ends here was `run` ticks, nb bits long; its middle stood at ph - 16 run: in lock 0 for an odd nb, 128 for an even
                const unsigned nb = (run + 4u) >> 3;
                if (nb >= 1u && run <= 96u) {
                    const unsigned err = (ph - 16u * run - ((nb & 1u) ? 0u : 128u)) & 255u;   // 1 ... 127: the clock is ahead; 128 ... 255: behind
                    if (err < 128u) ph = (ph - min(pull, err)) & 255u;
                    else ph = (ph + min(pull, 256u - err)) & 255u;
                }
                run = 0u;
            }
            if (run < 255u) run++;
            prev_s = s;
            ph += 32u;
            if (ph >= 256u) {
                ph -= 256u;
                bits++;
                sh = (sh >> 1) | (s << 15);
                if (!synced) {
                    if (sh == 0xABABu) { synced = 1u; syncs++; nbit = 0u; msg_len = 0u; head = 0u; sync_tick = k; }
                } else if (++nbit == 8u) {
                    nbit = 0u;
                    const unsigned byte = sh >> 8;
                    if (!(byte == 0xABu && msg_len == 0u)) {
                        const bool valid = (byte >= 0x20u && byte <= 0x7Eu) || byte == 0x0Du || byte == 0x0Au;
                        if (valid) {
                            if (lane == 0) st->msg[msg_len] = (unsigned char)byte;
                            if (msg_len < 4u) head |= byte << (8u * msg_len);
                            msg_len++;
                        }
                        if (!valid || msg_len == (unsigned)FMD_SAME_MAX_BYTES) {
                            const unsigned kind = msg_len < 4u ? 0u : (head == kZCZC ? (unsigned)FMD_SAME_KIND_HEADER : (head == kNNNN ? (unsigned)FMD_SAME_KIND_EOM : 0u));
                            if (kind) {
                                if (lane == 0) {
                                    fmd_same_message* rg = &st->ring[accepted & 7ull];
                                    rg->sync_tick = sync_tick;
                                    rg->len = (unsigned short)msg_len;
                                    rg->kind = (unsigned char)kind;
                                    rg->reserved = 0;
                                    for (unsigned i = 0; i < (unsigned)FMD_SAME_MAX_BYTES; i++) rg->bytes[i] = i < msg_len ? st->msg[i] : (unsigned char)0;
                                }
                                accepted++;
                                last_accept = k;
                                flags = kind == (unsigned)FMD_SAME_KIND_HEADER ? (flags | FMD_SAME_ALERT_OPEN) : (flags & ~FMD_SAME_ALERT_OPEN);
                            } else {
                                rejected++;
                            }
                            synced = 0u; msg_len = 0u; head = 0u;
                        }
                    }
                }
            }
            if ((flags & FMD_SAME_ALERT_OPEN) && k - last_accept >= (unsigned long long)hold) flags &= ~FMD_SAME_ALERT_OPEN;
        }

        if (nc < kT) {
#pragma unroll
            for (int k = 0; k < 4; k++) open[k] = sums[k][kSameHist + nc];   // the tick left open (+0 where it has no frame yet)
        }
        if (nc > 0) {                                                        // the newest seven ticks move to the front
            double v[4] = {0.0, 0.0, 0.0, 0.0};
            if (lane < kSameHist) {
#pragma unroll
                for (int k = 0; k < 4; k++) v[k] = sums[k][nc + lane];
            }
            __syncthreads();
            if (lane < kSameHist) {
#pragma unroll
                for (int k = 0; k < 4; k++) sums[k][lane] = v[k];
            }
        }
        done += (unsigned)nc;
        if (nc < kT) break;
        j0 += (unsigned)kT;
        acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
    }
    __syncthreads();

    if (lane == 0) {
        flags = (flags & ~FMD_SAME_SYNCED) | (synced ? FMD_SAME_SYNCED : 0u);
        const uint8_t ok = (uint8_t)((flags & alarm_mask) == 0u);
        st->frames = F0 + (unsigned long long)n;
        st->ticks = T0 + (unsigned long long)done;
        st->bits = bits; st->syncs = syncs; st->accepted = accepted; st->rejected = rejected;
        st->sync_tick = sync_tick; st->last_accept_tick = last_accept;
#pragma unroll
        for (int k = 0; k < 4; k++) st->open[k] = open[k];
#pragma unroll
        for (int h = 0; h < kSameHist; h++)
#pragma unroll
            for (int k = 0; k < 4; k++) st->hist[h][k] = sums[k][h];
        st->ph = ph; st->sh = sh; st->nbit = nbit; st->msg_len = msg_len; st->run = run;
        st->synced = (unsigned char)synced; st->prev_s = (unsigned char)prev_s;
        st->flags = (unsigned char)flags; st->ok = ok;
        if (out_flags) out_flags[c] = (uint8_t)flags;
        if (out_ok) out_ok[c] = ok;
    }
}

// stations c0 ... as after create (everything 0, every flag clear, ok = 1)
__global__ __launch_bounds__(kT) void k_same_reset(int c0, fmd_same_status* __restrict__ status) {
    const int c = c0 + blockIdx.x, t = threadIdx.x;
    fmd_same_status* st = status + c;
    unsigned* w = reinterpret_cast<unsigned*>(st);
    for (int i = t; i < (int)(sizeof(fmd_same_status) / 4); i += kT) w[i] = 0u;
    __syncthreads();
    if (t == 0) st->ok = 1;
}

// the parameters of stations c0 ...
__global__ __launch_bounds__(kT) void k_same_set(int c0, int cn, fmd_same_params p, fmd_same_params* __restrict__ prm, fmd_same_status* __restrict__ status) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= cn) return;
    fmd_same_status* st = status + c0 + i;
    prm[c0 + i] = p;
    st->ok = (unsigned char)((st->flags & p.alarm_mask) == 0);
}

}  // namespace

struct fmd_same_s {
    int C = 0, fs = 0;
    fmd::SameGeometry geo{};
    long long max_in = 0;
    std::vector<fmd_same_params> params;     // [C], as set
    fmd_same_status* d_status = nullptr;     // [C]
    fmd_same_params* d_prm = nullptr;        // [C]
    double2* d_tab = nullptr;                // [P]: cos, sin of 2 pi j / P
    fmd::CallOrder order;                    // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int sm_fail(fmd_same d, int code, const char* fmt, A... args) { return fmd::fail(d ? d->err : fmd::same_global_error(), code, fmt, args...); }

extern "C" {

int fmd_same_create(const fmd_same_config* cfg, fmd_same* out) {
    if (!cfg || !out) return sm_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->n_channels <= 0 || cfg->max_input_frames <= 0 || cfg->max_input_frames > (1LL << 30))
        return sm_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_frames %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_frames);
    fmd::SameGeometry geo;
    if (!fmd::same_geometry(cfg->fs, &geo)) return sm_fail(nullptr, FMD_ERR_ARG, "fs %d is not a multiple of 10 in 8000 ... 48000", cfg->fs);
    if (fmd_device_count() <= 0) return sm_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return sm_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_same d = new fmd_same_s();
    d->C = cfg->n_channels; d->fs = cfg->fs; d->geo = geo; d->max_in = cfg->max_input_frames;
    fmd_same_params p{};
    fmd_same_default_params(&p);
    d->params.assign((size_t)d->C, p);
    const size_t C = (size_t)d->C;
    std::vector<double> tab(2 * (size_t)geo.P);
    fmd::same_table(geo.P, tab.data());
    bool ok = d->order.init(dev);
    ok = ok && hipMalloc(&d->d_status, sizeof(fmd_same_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&d->d_prm, sizeof(fmd_same_params) * C) == hipSuccess;
    ok = ok && hipMalloc(&d->d_tab, sizeof(double) * tab.size()) == hipSuccess;
    ok = ok && hipMemset(d->d_prm, 0, sizeof(fmd_same_params) * C) == hipSuccess;
    ok = ok && hipMemcpy(d->d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice) == hipSuccess;
    // (the reset first: set_params reads the record's flags)
    if (!ok || fmd_same_reset(d, -1) != FMD_OK || fmd_same_set_params(d, -1, &p) != FMD_OK) {
        fmd_same_destroy(d);
        return sm_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed");
    }
    *out = d;
    return FMD_OK;
}

int fmd_same_destroy(fmd_same d) {
    if (!d) return FMD_ERR_ARG;
    (void)d->order.quiesce();
    for (void* p : {(void*)d->d_status, (void*)d->d_prm, (void*)d->d_tab})
        if (p) (void)hipFree(p);
    delete d;
    return FMD_OK;
}

int fmd_same_reset(fmd_same d, int channel) {
    if (!d) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, d->C, &c0, &cn)) return sm_fail(d, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, d->C);
    if (!d->order.quiesce()) return sm_fail(d, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_same_reset, dim3((unsigned)cn), dim3(kT), 0, nullptr, c0, d->d_status);
    if (const char* e = fmd::control_end("k_same_reset launch failed")) return sm_fail(d, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;                                                           // (the parameters are kept; with every flag clear ok = 1 whatever the mask)
}

int fmd_same_set_params(fmd_same d, int channel, const fmd_same_params* p) {
    if (!d) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, d->C, &c0, &cn)) return sm_fail(d, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, d->C);
    if (fmd::same_check_params(p, &d->err) != FMD_OK) return FMD_ERR_ARG;
    if (!d->order.quiesce()) return sm_fail(d, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_same_set, dim3((unsigned)((cn + kT - 1) / kT)), dim3(kT), 0, nullptr, c0, cn, *p, d->d_prm, d->d_status);
    if (const char* e = fmd::control_end("k_same_set launch failed")) return sm_fail(d, FMD_ERR_DEVICE, "%s", e);
    for (int c = c0; c < c0 + cn; c++) d->params[(size_t)c] = *p;
    return FMD_OK;
}

int fmd_same_get_params(fmd_same d, int channel, fmd_same_params* p) {
    if (!d || !p) return sm_fail(d, FMD_ERR_ARG, "null decoder or output");
    if (channel < 0 || channel >= d->C) return sm_fail(d, FMD_ERR_ARG, "channel %d outside [0, %d)", channel, d->C);
    *p = d->params[(size_t)channel];
    return FMD_OK;
}

int fmd_same_process_f32_dev(fmd_same d, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_flags, uint8_t* d_ok,
                             void* stream) {
    if (!d) return FMD_ERR_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return sm_fail(d, FMD_ERR_ARG, "null input, or input not aligned to 8 bytes");
    if (n < 0 || n > in_stride || n > d->max_in)
        return sm_fail(d, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or above max_input_frames %lld", n, in_stride, d->max_in);
    if (n == 0 && !d_flags && !d_ok) return FMD_OK;                          // nothing of any station changes and there is no byte to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* e = d->order.begin(s)) return sm_fail(d, FMD_ERR_DEVICE, "%s", e);
    hipLaunchKernelGGL(k_same, dim3((unsigned)d->C), dim3(kT), 0, s, reinterpret_cast<const float2*>(d_in), in_stride, n, d_active, d->fs, d->geo.P,
                       d->geo.mark_step, d->geo.space_step, d->d_tab, d->d_prm, d->d_status, d_flags, d_ok);
    if (hipGetLastError() != hipSuccess) return sm_fail(d, FMD_ERR_DEVICE, "k_same launch failed");
    if (const char* e = d->order.end(s)) return sm_fail(d, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_same_get_status(fmd_same d, fmd_same_status* out) {
    if (!d || !out) return sm_fail(d, FMD_ERR_ARG, "null decoder or output");
    if (!d->order.quiesce()) return sm_fail(d, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, d->d_status, sizeof(fmd_same_status) * (size_t)d->C, hipMemcpyDeviceToHost) != hipSuccess) return sm_fail(d, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_same_status_dev(fmd_same d, const fmd_same_status** d_status) {
    if (!d || !d_status) return sm_fail(d, FMD_ERR_ARG, "null decoder or output");
    *d_status = d->d_status;
    return FMD_OK;
}

const char* fmd_same_last_error(fmd_same d) { return d ? d->err.c_str() : fmd::same_global_error().c_str(); }

}  // extern "C"
