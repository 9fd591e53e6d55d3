// ADPCM audio encoder, device side (include/fmdemod.h, "ADPCM audio encoder").
//
// NOT in the reference.  Block IMA / DVI ADPCM of the station audio [C][in_stride][2] f32 that the mixer and the monitors read, read in
// place: per station a stream of blocks of S frames, 4 bits a sample, written to a caller-owned device array as the blocks complete.
//
// Each (station, rail) is a serial chain of integer operations with no parallelism inside it, so k_adpcm gives a chain a lane: one
// wavefront per group of 32 stations, lane l = station l & 31, rail l >> 5 (a station's two rails sit in the two halves of the
// wavefront, which an LDS read serves apart: they read the same word and it costs nothing).  The lanes do not walk their own rows.
// Per tile of 128 frames the wavefront loads the group's rows cooperatively, one 16-byte non-temporal load per station and lane (a
// station's 1 KB of the tile per instruction), converts to q at once, packs (qL, qR) into one word and stores the words to LDS as
// [station][frame] with a row stride of 129 words, so that the 32 stations of a column read fall into 32 banks.  The next tile's loads
// are issued into registers (32 x 16 bytes a lane) before the chains run over the tile at hand, eight words of the lane's row per LDS
// read batch.  The block's header frame is a predicated branch per lane: stations stand at different places in their blocks.  The step
// table lives in LDS as 89 x 16 bytes, entry i holding the five steps that index i can move to; the entry is read at a frame's start
// and the next step chosen by the code at its end, so that the table's latency does not sit in the chain.  Each lane packs eight codes
// into one word and stores it directly, with an ordinary store: to the caller's array where the block completes within the call, else
// to the encoder's open block, whose earlier words the lane copies across when the block does complete.  Clamped and non-finite samples
// are counted where they are converted, by wave-wide ballots behind one test that is false for clean audio.  A frame outside the
// validated n is neither loaded nor encoded.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "fmd_adpcm_design.h"
#include "fmd_side.h"
#include "fmdemod.h"

using fmd::kAdpcmSteps;

namespace {

constexpr int kT = 64;               // threads per workgroup: one wavefront
constexpr int kSt = 32;              // stations per wavefront: 64 chains
constexpr int kTile = 128;           // frames per tile: two per lane and station row
constexpr int kRow = kTile + 1;      // words per station row in LDS
static_assert(kTile == 2 * kT && kSt * 2 == kT, "k_adpcm's lane layout");

static_assert(sizeof(fmd_adpcm_status) == 64 && offsetof(fmd_adpcm_status, blocks) == 8 && offsetof(fmd_adpcm_status, padded) == 16 &&
              offsetof(fmd_adpcm_status, clipped) == 24 && offsetof(fmd_adpcm_status, nonfinite) == 40 && offsetof(fmd_adpcm_status, fill) == 48 &&
              offsetof(fmd_adpcm_status, pred) == 52 && offsetof(fmd_adpcm_status, index) == 56 && offsetof(fmd_adpcm_status, reserved) == 58,
              "fmd_adpcm_status layout");

__constant__ unsigned short c_step[kAdpcmSteps] = {FMD_ADPCM_STEP_TABLE};

// what the encoder keeps per station beside its record: each rail's open code word, and the last real frame's (qL, qR)
struct AdPriv { uint32_t acc[2], lastq, reserved; };

typedef float ad_f4 __attribute__((ext_vector_type(4), aligned(8)));         // a station's rows are aligned to a frame only
typedef float ad_f2 __attribute__((ext_vector_type(2)));

// the contract's sample: q, and whether it was clamped or not finite
__device__ __forceinline__ int ad_q(float x, bool& clip, bool& nonf) {
    const float t = x * (32767.0f * 0.95f);
    clip = false;
    nonf = !(fabsf(t) <= 3.402823466e38f);
    if (nonf) return 0;
    if (t >= 32768.0f) { clip = true; return 32767; }                        // (int)t > 32767
    if (t <= -32769.0f) { clip = true; return -32768; }                      // (int)t < -32768
    return (int)t;
}

// s_nx[i] = the steps at the five indices that index i moves to: {i - 1 | i + 2 << 16, i + 4 | i + 6 << 16, i + 8, i}, clamped to 0 ... 88
__device__ __forceinline__ void ad_table(uint4* s_nx, int lane) {
    for (int i = lane; i < kAdpcmSteps; i += kT) {
        auto at = [](int k) { return (unsigned)c_step[k < 0 ? 0 : k > 88 ? 88 : k]; };
        s_nx[i] = make_uint4(at(i - 1) | (at(i + 2) << 16), at(i + 4) | (at(i + 6) << 16), at(i + 8), at(i));
    }
}

// a chain: one rail of one station
struct AdChain {
    int fill, pred, index, step;     // frames in the open block; the predictor; the step index and table[index]
    uint32_t acc;                    // the code word being packed
    int togo;                        // blocks that this call still completes
    uint32_t* dst;                   // the open block's word 0 of this rail: in the caller's array while togo > 0, else in the encoder's
    uint32_t* open;
    int align_w;                     // words of a block
};

// one frame of the chain
__device__ __forceinline__ void ad_frame(AdChain& ch, int q, int S, const uint4* s_nx) {
    if (ch.fill == 0) {                                                      // the block's header: the sample itself, the index as it stands
        ch.pred = q;
        ch.dst[0] = ((uint32_t)q & 0xffffu) | ((uint32_t)ch.index << 16);
        ch.fill = 1;
        return;
    }
    const uint4 nx = s_nx[ch.index];                                         // (in flight while the code is made)
    const int step = ch.step;
    int diff = q - ch.pred;
    uint32_t code = diff < 0 ? 8u : 0u;
    diff = diff < 0 ? -diff : diff;
    int vp = step >> 3;
    if (diff >= step) { code |= 4u; diff -= step; vp += step; }
    const int s1 = step >> 1;
    if (diff >= s1) { code |= 2u; diff -= s1; vp += s1; }
    const int s2 = step >> 2;
    if (diff >= s2) { code |= 1u; vp += s2; }
    int pred = (code & 8u) ? ch.pred - vp : ch.pred + vp;
    ch.pred = pred > 32767 ? 32767 : pred < -32768 ? -32768 : pred;
    const int m = (int)(code & 7u);
    const int index = m < 4 ? ch.index - 1 : ch.index + 2 * m - 6;
    ch.index = index < 0 ? 0 : index > 88 ? 88 : index;
    // the next step: half-word k = 0 ... 4 of the entry, by selects and a shift (written as a chain of comparisons on m the compiler
    // makes it a switch: four nested divergent branches a frame)
    const uint32_t k5 = (uint32_t)(m < 4 ? 0 : m - 3);
    const uint32_t w01 = (k5 & 2u) ? nx.y : nx.x;
    const uint32_t wk = (k5 & 4u) ? nx.z : w01;
    ch.step = (int)((wk >> ((k5 & 1u) << 4)) & 0xffffu);
    const int k = ch.fill - 1;                                               // the code's place: word k / 8 + 1 of the rail, nibble k % 8
    ch.acc |= code << (4 * (k & 7));
    if ((k & 7) == 7) {
        ch.dst[2 * ((k >> 3) + 1)] = ch.acc;
        ch.acc = 0u;
    }
    if (++ch.fill == S) {                                                    // (S = 1 mod 8: the block's last word has just been stored)
        ch.fill = 0;
        ch.togo--;
        ch.dst = ch.togo > 0 ? ch.dst + ch.align_w : ch.open;
    }
}

// the open block's words of this rail that the encoder holds, into the caller's array, where the block completes within the call
__device__ __forceinline__ void ad_carry_open(const AdChain& ch) {
    const int words = 1 + ((ch.fill - 1) >> 3);                              // the header and the full code words
    for (int g = 0; g < words; g++) ch.dst[2 * g] = ch.open[2 * g];
}

// in [C][in_stride] frames (L, R); status, priv [C]; open [C][align / 4] words; out: station c's blocks from word c * out_stride_w on
__global__ __launch_bounds__(kT) void k_adpcm(const float2* __restrict__ in, long long in_stride, int n, const uint8_t* __restrict__ active, int C, int S,
                                              int align_w, fmd_adpcm_status* __restrict__ status, AdPriv* __restrict__ priv, uint32_t* __restrict__ open,
                                              uint32_t* __restrict__ out, long long out_stride_w, int* __restrict__ nblocks) {
    __shared__ uint4 s_nx[kAdpcmSteps];
    __shared__ uint32_t s_q[kSt * kRow];
    const int lane = threadIdx.x, st = lane & (kSt - 1), rail = lane >> 5;
    const int c0 = blockIdx.x * kSt, c = c0 + st;
    const bool live = c < C && (!active || active[c] != 0);
    if (c < C && !live && rail == 0 && nblocks) nblocks[c] = 0;              // a skipped station
    const unsigned long long amask = __ballot(live);                         // bit s (and s + 32): station c0 + s takes part
    if (amask == 0ull) return;                                               // (uniform)
    ad_table(s_nx, lane);

    fmd_adpcm_status* stp = status + c;                                      // (dereferenced by live lanes only)
    AdChain ch{};
    int nb = 0;
    if (live) {
        ch.fill = (int)stp->fill; ch.pred = stp->pred[rail]; ch.index = stp->index[rail]; ch.step = c_step[ch.index];
        ch.acc = priv[c].acc[rail];
        nb = (int)(((long long)ch.fill + n) / S);                            // (n <= 2^30)
        ch.togo = nb; ch.align_w = align_w;
        ch.open = open + (size_t)c * (size_t)align_w + rail;
        ch.dst = nb > 0 ? out + (size_t)c * (size_t)out_stride_w + rail : ch.open;
        if (nb > 0 && ch.fill > 0) ad_carry_open(ch);
    }
    unsigned clipped = 0u, nonfinite = 0u;                                   // of the lane's own station: this call's
    const float2* base = in + (size_t)c0 * (size_t)in_stride + 2 * lane;

    // the lane's two frames of every station's row of a tile; a frame outside the call reads as (+0, +0): q = 0, not counted, not encoded
    ad_f4 nxt[kSt];
    auto fetch = [&](int t0) {
        const int i = t0 + 2 * lane;
#pragma unroll
        for (int s = 0; s < kSt; s++) {
            if (!((amask >> s) & 1ull)) continue;                            // (uniform)
            const float2* p = base + (size_t)s * (size_t)in_stride + t0;
            ad_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (i + 1 < n) v = __builtin_nontemporal_load(reinterpret_cast<const ad_f4*>(p));
            else if (i < n) {
                const ad_f2 a = __builtin_nontemporal_load(reinterpret_cast<const ad_f2*>(p));
                v.x = a.x; v.y = a.y;
            }
            nxt[s] = v;
        }
    };

    fetch(0);
    for (int t0 = 0; t0 < n; t0 += kTile) {
        const int len = n - t0 < kTile ? n - t0 : kTile;
        __syncthreads();                                                     // the table is there; the chains are through with the tile before
#pragma unroll
        for (int s = 0; s < kSt; s++) {
            if (!((amask >> s) & 1ull)) continue;                            // (uniform)
            bool cl[4], nf[4];
            const int q0 = ad_q(nxt[s].x, cl[0], nf[0]), q1 = ad_q(nxt[s].y, cl[1], nf[1]);
            const int q2 = ad_q(nxt[s].z, cl[2], nf[2]), q3 = ad_q(nxt[s].w, cl[3], nf[3]);
            s_q[s * kRow + 2 * lane] = ((uint32_t)q0 & 0xffffu) | ((uint32_t)q1 << 16);
            s_q[s * kRow + 2 * lane + 1] = ((uint32_t)q2 & 0xffffu) | ((uint32_t)q3 << 16);
            const bool any = cl[0] | cl[1] | cl[2] | cl[3] | nf[0] | nf[1] | nf[2] | nf[3];
            if (__ballot(any) != 0ull) {                                     // (uniform; false for clean audio)
                const unsigned l = (unsigned)(__popcll(__ballot(cl[0])) + __popcll(__ballot(cl[2])));
                const unsigned r = (unsigned)(__popcll(__ballot(cl[1])) + __popcll(__ballot(cl[3])));
                const unsigned f = (unsigned)(__popcll(__ballot(nf[0])) + __popcll(__ballot(nf[1])) + __popcll(__ballot(nf[2])) + __popcll(__ballot(nf[3])));
                if (st == s) { clipped += rail ? r : l; nonfinite += f; }
            }
        }
        if (t0 + kTile < n) fetch(t0 + kTile);                               // in flight while the chains run
        __syncthreads();
        if (live) {
            const uint32_t* row = s_q + st * kRow;
            for (int f0 = 0; f0 < len; f0 += 8) {
                uint32_t w[8];
#pragma unroll
                for (int j = 0; j < 8; j++) w[j] = row[f0 + j];              // (f0 + j < kTile)
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if (f0 + j < len) ad_frame(ch, (int)(w[j] << (rail ? 0 : 16)) >> 16, S, s_nx);   // (uniform test)
            }
        }
    }

    if (live) {
        stp->pred[rail] = (short)ch.pred;
        stp->index[rail] = (unsigned char)ch.index;
        stp->clipped[rail] += clipped;
        priv[c].acc[rail] = ch.acc;
        if (rail == 0) {
            stp->frames += (unsigned long long)n;
            stp->blocks += (unsigned long long)nb;
            stp->nonfinite += nonfinite;
            stp->fill = (unsigned)ch.fill;
            if (n > 0) priv[c].lastq = s_q[st * kRow + ((n - 1) & (kTile - 1))];
            if (nblocks) nblocks[c] = nb;
        }
    }
}

// stations c0 ... c0 + cn - 1: the open block closed with repeats of the last real frame
__global__ __launch_bounds__(kT) void k_adpcm_flush(int c0, int cn, int S, int align_w, fmd_adpcm_status* __restrict__ status, AdPriv* __restrict__ priv,
                                                    uint32_t* __restrict__ open, uint32_t* __restrict__ out, long long out_stride_w, int* __restrict__ nblocks) {
    __shared__ uint4 s_nx[kAdpcmSteps];
    const int lane = threadIdx.x, st = lane & (kSt - 1), rail = lane >> 5;
    const int i = blockIdx.x * kSt + st, c = c0 + i;
    ad_table(s_nx, lane);
    __syncthreads();
    if (i >= cn) return;
    fmd_adpcm_status* stp = status + c;
    const int fill = (int)stp->fill;
    if (fill == 0) {
        if (rail == 0 && nblocks) nblocks[c] = 0;
        return;
    }
    AdChain ch{};
    ch.fill = fill; ch.pred = stp->pred[rail]; ch.index = stp->index[rail]; ch.step = c_step[ch.index];
    ch.acc = priv[c].acc[rail];
    ch.togo = 1; ch.align_w = align_w;
    ch.open = open + (size_t)c * (size_t)align_w + rail;
    ch.dst = out + (size_t)c * (size_t)out_stride_w + rail;
    ad_carry_open(ch);
    const uint32_t w = priv[c].lastq;
    const int q = (int)(w << (rail ? 0 : 16)) >> 16;
    for (int k = fill; k < S; k++) ad_frame(ch, q, S, s_nx);
    stp->pred[rail] = (short)ch.pred;
    stp->index[rail] = (unsigned char)ch.index;
    priv[c].acc[rail] = ch.acc;                                              // (0: the block is complete)
    if (rail == 0) {
        stp->padded += (unsigned long long)(S - fill);
        stp->blocks += 1ull;
        stp->fill = 0u;
        if (nblocks) nblocks[c] = 1;
    }
}

// stations c0 ... c0 + cn - 1 as after create
__global__ __launch_bounds__(kT) void k_adpcm_reset(int c0, int cn, fmd_adpcm_status* __restrict__ status, AdPriv* __restrict__ priv) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= cn) return;
    uint4* w = reinterpret_cast<uint4*>(status + c0 + i);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(fmd_adpcm_status) / 16); k++) w[k] = make_uint4(0u, 0u, 0u, 0u);
    *reinterpret_cast<uint4*>(priv + c0 + i) = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

struct fmd_adpcm_s {
    int C = 0, S = 0, align = 0;
    long long max_in = 0;
    fmd_adpcm_status* d_status = nullptr;    // [C]
    AdPriv* d_priv = nullptr;                // [C]
    uint32_t* d_open = nullptr;              // [C][align / 4]: each station's open block
    fmd::CallOrder order;                    // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int ad_fail(fmd_adpcm e, int code, const char* fmt, A... args) { return fmd::fail(e ? e->err : fmd::adpcm_global_error(), code, fmt, args...); }

extern "C" {

int fmd_adpcm_create(const fmd_adpcm_config* cfg, fmd_adpcm* out) {
    if (!cfg || !out) return ad_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->n_channels <= 0 || cfg->max_input_frames <= 0 || cfg->max_input_frames > (1LL << 30))
        return ad_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_frames %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_frames);
    const int S = fmd::adpcm_block_frames(cfg->block_frames);
    if (S == 0) return ad_fail(nullptr, FMD_ERR_ARG, "block_frames %d is neither 0 nor 1 (mod 8) in 9 ... 8185", cfg->block_frames);
    if (fmd_device_count() <= 0) return ad_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return ad_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_adpcm e = new fmd_adpcm_s();
    e->C = cfg->n_channels; e->S = S; e->align = fmd::adpcm_block_align(S); e->max_in = cfg->max_input_frames;
    const size_t C = (size_t)e->C;
    bool ok = e->order.init(dev);
    ok = ok && hipMalloc(&e->d_status, sizeof(fmd_adpcm_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&e->d_priv, sizeof(AdPriv) * C) == hipSuccess;
    ok = ok && hipMalloc(&e->d_open, (size_t)e->align * C) == hipSuccess;
    ok = ok && hipMemset(e->d_open, 0, (size_t)e->align * C) == hipSuccess;
    if (!ok || fmd_adpcm_reset(e, -1) != FMD_OK) {
        fmd_adpcm_destroy(e);
        return ad_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed");
    }
    *out = e;
    return FMD_OK;
}

int fmd_adpcm_destroy(fmd_adpcm e) {
    if (!e) return FMD_ERR_ARG;
    (void)e->order.quiesce();
    for (void* p : {(void*)e->d_status, (void*)e->d_priv, (void*)e->d_open})
        if (p) (void)hipFree(p);
    delete e;
    return FMD_OK;
}

int fmd_adpcm_reset(fmd_adpcm e, int channel) {
    if (!e) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, e->C, &c0, &cn)) return ad_fail(e, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, e->C);
    if (!e->order.quiesce()) return ad_fail(e, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_adpcm_reset, dim3((unsigned)((cn + kT - 1) / kT)), dim3(kT), 0, nullptr, c0, cn, e->d_status, e->d_priv);
    if (const char* m = fmd::control_end("k_adpcm_reset launch failed")) return ad_fail(e, FMD_ERR_DEVICE, "%s", m);
    return FMD_OK;
}

int fmd_adpcm_process_f32_dev(fmd_adpcm e, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_out, long long out_stride,
                              int* d_nblocks, void* stream) {
    if (!e) return FMD_ERR_ARG;
    if (fmd::adpcm_check_call(e->S, e->max_in, d_in, in_stride, n, d_out, out_stride, &e->err) != FMD_OK) return FMD_ERR_ARG;
    if (n == 0 && !d_nblocks) return FMD_OK;                                 // nothing of any station changes and there is no count to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* m = e->order.begin(s)) return ad_fail(e, FMD_ERR_DEVICE, "%s", m);
    hipLaunchKernelGGL(k_adpcm, dim3((unsigned)((e->C + kSt - 1) / kSt)), dim3(kT), 0, s, reinterpret_cast<const float2*>(d_in), in_stride, (int)n, d_active, e->C,
                       e->S, e->align / 4, e->d_status, e->d_priv, e->d_open, reinterpret_cast<uint32_t*>(d_out), out_stride / 4, d_nblocks);
    if (hipGetLastError() != hipSuccess) return ad_fail(e, FMD_ERR_DEVICE, "k_adpcm launch failed");
    if (const char* m = e->order.end(s)) return ad_fail(e, FMD_ERR_DEVICE, "%s", m);
    return FMD_OK;
}

int fmd_adpcm_flush(fmd_adpcm e, int channel, uint8_t* d_out, long long out_stride, int* d_nblocks, void* stream) {
    if (!e) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, e->C, &c0, &cn)) return ad_fail(e, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, e->C);
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 4 != 0) return ad_fail(e, FMD_ERR_ARG, "null output, or output not aligned to 4 bytes");
    if (out_stride % 4 != 0 || out_stride < e->align)
        return ad_fail(e, FMD_ERR_ARG, "out_stride %lld is no multiple of 4 or below the block's %d bytes", out_stride, e->align);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const char* m = e->order.begin(s)) return ad_fail(e, FMD_ERR_DEVICE, "%s", m);
    hipLaunchKernelGGL(k_adpcm_flush, dim3((unsigned)((cn + kSt - 1) / kSt)), dim3(kT), 0, s, c0, cn, e->S, e->align / 4, e->d_status, e->d_priv, e->d_open,
                       reinterpret_cast<uint32_t*>(d_out), out_stride / 4, d_nblocks);
    if (hipGetLastError() != hipSuccess) return ad_fail(e, FMD_ERR_DEVICE, "k_adpcm_flush launch failed");
    if (const char* m = e->order.end(s)) return ad_fail(e, FMD_ERR_DEVICE, "%s", m);
    return FMD_OK;
}

int fmd_adpcm_get_status(fmd_adpcm e, fmd_adpcm_status* out) {
    if (!e || !out) return ad_fail(e, FMD_ERR_ARG, "null encoder or output");
    if (!e->order.quiesce()) return ad_fail(e, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, e->d_status, sizeof(fmd_adpcm_status) * (size_t)e->C, hipMemcpyDeviceToHost) != hipSuccess) return ad_fail(e, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_adpcm_status_dev(fmd_adpcm e, const fmd_adpcm_status** d_status) {
    if (!e || !d_status) return ad_fail(e, FMD_ERR_ARG, "null encoder or output");
    *d_status = e->d_status;
    return FMD_OK;
}

const char* fmd_adpcm_last_error(fmd_adpcm e) { return e ? e->err.c_str() : fmd::adpcm_global_error().c_str(); }

}  // extern "C"
