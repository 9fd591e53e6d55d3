// Audio fingerprinter, device side (include/fmdemod.h, "Audio fingerprinter").
//
// NOT in the reference.  Per station the mono signal m = 0.5f (L + R) of the station audio [C][in_stride][2] f32 that the mixer and the
// monitors read, read in place; per completed hop-sized sub-block its K-bin spectrum as two fmaf chains in ascending n; per frame of
// R sub-blocks the bins as fmaf chains over R twiddles, the Hann window as three taps, the powers, the band energies in ascending k and
// against the frame before the 32-bit word.
//
// Three kernels a piece of a call (a call of no more than FprintLayout::piece_frames frames is one piece):
//   k_fprint_map    one workgroup: the sub-blocks each station completes, as an exclusive prefix sum: the rows of the GEMM (the scan and
//                   its inverse, row -> station, are fmd_rowmap.h's, shared with the matcher).
//   k_fprint_sub    the sub-block transform of the whole batch as ONE dense GEMM on v_mfma_f32_16x16x4_f32: rows are (station, sub-block)
//                   pairs, columns the re and the im of the Kp bins, the depth runs over n in ascending order through the accumulator
//                   from a zero C, which is a k-ordered fmaf chain with one rounding per product.  The A operand is formed
//                   where it is read, from the carried samples and the caller's audio; the B operand is read from the design-time image
//                   [H][2 Kp] in global memory, which every workgroup shares.  A workgroup is four wavefronts on the same 64 rows, each
//                   with its own 64 columns: 16 accumulators a wavefront, four A and four B values a step.  Sub-blocks do not overlap,
//                   so all row tiles but the batch's last are full whatever the call length.  The spectra go to the scratch.
//   k_fprint_frame  one workgroup a station streams the bins in chunks of 64 (+ 1 on each side): reads the kept R - 1 spectra and the
//                   piece's new ones once into LDS, forms every new frame's X, the taps, P, adds to the band energies, and behind the
//                   last chunk takes the differences, packs the words, moves the newest R - 1 spectra into the ring and the unconsumed
//                   samples into the carry, and writes the record.
// No atomics, no register spills (scratch 0), no workgroup waits on another.
//
// Bounds: k_fprint_sub reads audio frames below the piece's n <= in_stride, carried samples below fill < H, image columns below 2 Kp and
// rows below H, and stores rows below rowbase[C] <= C * piece, the scratch's size.  k_fprint_frame's LDS rows lie below R - 1 + piece,
// its columns below 66, its frames below piece, bands below 33; ring slots are taken mod R - 1, bins lie below K <= Kp; words are
// stored below the call's count <= fmd_fprint_max_prints(hop, n) <= out_stride, energies likewise.
//
// Denormals: fp32 denormals are kept (hipcc's default mode; this file is NOT built with -fgpu-flush-denormals-to-zero).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fmd_fprint_design.h"
#include "fmd_rowmap.h"
#include "fmd_side.h"
#include "fmdemod.h"

using fmd::FprintLayout;
using fmd::kFprintChunk;
using fmd::kFprintMaxBands;
using fmd::kFprintTile;

namespace {

constexpr int kT = 256;              // threads per workgroup: four wavefronts
constexpr int kRT = 4;               // row tiles of a workgroup of k_fprint_sub (all four wavefronts work on them)
constexpr int kCT = 4;               // column tiles a wavefront works on
constexpr int kSpan = kFprintChunk + 2;
static_assert(kFprintTile == 16, "the 16x16x4 MFMA's tile");

static_assert(sizeof(fmd_fprint_status) == 32 && offsetof(fmd_fprint_status, prints) == 8 && offsetof(fmd_fprint_status, nonfinite) == 16 &&
              offsetof(fmd_fprint_status, fill) == 24 && offsetof(fmd_fprint_status, reserved) == 28, "fmd_fprint_status layout");

typedef float fp_f4 __attribute__((ext_vector_type(4)));

// what the kernels read of the configuration and the layout
struct FprintDev {
    int H, R, B, K, Kp, first, piece;
};

__device__ __forceinline__ unsigned fp_bits(float f) { return __float_as_uint(f); }
__device__ __forceinline__ bool fp_nonfinite(float f) { return (fp_bits(f) & 0x7f800000u) == 0x7f800000u; }

// rowbase [C + 1]: the exclusive prefix sum of the sub-blocks (fill + n) / H each active station completes
__global__ __launch_bounds__(fmd::rowmap::kThreads) void k_fprint_map(int C, long long n, const uint8_t* __restrict__ active,
                                                                     const fmd_fprint_status* __restrict__ status, int H, int* __restrict__ rowbase) {
    fmd::rowmap::scan(C, [&](int c) { return (active && active[c] == 0) ? 0 : (int)(((long long)status[c].fill + n) / H); }, rowbase);
}

// in [C][in_stride] frames (L, R); carry [C][H]; img [H][2 Kp]; scratch [rows][2 Kp]
template <bool kCarry>
__device__ __forceinline__ void fp_gemm(fp_f4 (&acc)[kRT][kCT], const float2* (&ip)[kRT], const float* (&cp)[kRT], int (&fr)[kRT],
                                        const float* __restrict__ bp, int H, int ld, int cnt) {
    for (int n0 = 0; n0 < H; n0 += 4) {
        float a[kRT], b[kCT];
#pragma unroll
        for (int i = 0; i < kRT; i++) {
            if (kCarry && n0 < fr[i]) {
                a[i] = cp[i][n0];
            } else {
                const float2 v = ip[i][n0];
                a[i] = 0.5f * (v.x + v.y);
            }
        }
#pragma unroll
        for (int j = 0; j < kCT; j++) b[j] = j < cnt ? bp[(size_t)n0 * (size_t)ld + j * kFprintTile] : 0.0f;
#pragma unroll
        for (int i = 0; i < kRT; i++)
#pragma unroll
            for (int j = 0; j < kCT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

__global__ __launch_bounds__(kT) void k_fprint_sub(const float2* __restrict__ in, long long in_stride, int C, FprintDev g, const int* __restrict__ rowbase,
                                                   const fmd_fprint_status* __restrict__ status, const float* __restrict__ carry, const float* __restrict__ img,
                                                   float* __restrict__ scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int M = rowbase[C];
    const int row0 = blockIdx.x * (kRT * kFprintTile);
    if (row0 >= M) return;
    const int ld = 2 * g.Kp, ntiles = ld / kFprintTile;
    const int ct0 = (blockIdx.y * (kT / 64) + wave) * kCT;
    if (ct0 >= ntiles) return;                                               // (no barrier in this kernel)
    const int cnt = min(kCT, ntiles - ct0);

    const float2* ip[kRT];
    const float* cp[kRT];
    int fr[kRT];
    bool any = false;
#pragma unroll
    for (int i = 0; i < kRT; i++) {
        const int r = min(row0 + i * kFprintTile + col, M - 1);              // a row past the batch repeats its last
        const int c = fmd::rowmap::owner(rowbase, C, r), sub = r - rowbase[c];   // the station: rowbase[c] <= r < rowbase[c + 1]
        const int fill = (int)status[c].fill;
        const long long q0 = (long long)sub * g.H + kq;                      // this lane's first sample, counted from the carry's start
        fr[i] = (int)(fill - q0);                                            // samples n0 below this come from the carry
        cp[i] = carry + (size_t)c * (size_t)g.H + (size_t)q0;
        ip[i] = in + (size_t)c * (size_t)in_stride + (q0 - fill);            // (dereferenced from n0 = fr on only)
        any = any || fr[i] > 0;
    }
    fp_f4 acc[kRT][kCT];
#pragma unroll
    for (int i = 0; i < kRT; i++)
#pragma unroll
        for (int j = 0; j < kCT; j++) acc[i][j] = fp_f4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* bp = img + (size_t)kq * (size_t)ld + (size_t)(ct0 * kFprintTile + col);
    if (__any(any)) fp_gemm<true>(acc, ip, cp, fr, bp, g.H, ld, cnt);
    else fp_gemm<false>(acc, ip, cp, fr, bp, g.H, ld, cnt);
#pragma unroll
    for (int i = 0; i < kRT; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = row0 + i * kFprintTile + kq * 4 + r;
            if (row < M) {
#pragma unroll
                for (int j = 0; j < kCT; j++)
                    if (j < cnt) scratch[(size_t)row * (size_t)ld + (size_t)((ct0 + j) * kFprintTile + col)] = acc[i][j][r];
            }
        }
}

// status, carry [C][H], ring [C][R - 1][2 Kp], elast [C][33], cnt [C]; out [C][out_stride]; nprints [C] or null; energy [C][energy_stride] or null
__global__ __launch_bounds__(kT) void k_fprint_frame(const float2* __restrict__ in, long long in_stride, long long n, const uint8_t* __restrict__ active, FprintDev g,
                                                     const int* __restrict__ rowbase, const float* __restrict__ scratch, const float* __restrict__ d_wc,
                                                     const float* __restrict__ d_ws, const int* __restrict__ d_edges, fmd_fprint_status* __restrict__ status,
                                                     float* __restrict__ carry_all, float* __restrict__ ring_all, float* __restrict__ elast_all, int* __restrict__ cnt_all,
                                                     int first_piece, int last_piece, uint32_t* __restrict__ out, long long out_stride, int* __restrict__ nprints,
                                                     float* __restrict__ energy, long long energy_stride) {
    extern __shared__ float lds[];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (active && active[c] == 0) return;                                    // (uniform over the workgroup)
    const int H = g.H, R = g.R, B = g.B, K = g.K, Kp = g.Kp, ld = 2 * g.Kp;
    float2* s_S = reinterpret_cast<float2*>(lds);                            // [R - 1 + piece][kSpan]
    float2* s_X = s_S + (size_t)(R - 1 + g.piece) * kSpan;                   // [piece][kSpan]
    float* s_P = reinterpret_cast<float*>(s_X + (size_t)g.piece * kSpan);    // [piece][kFprintChunk]; behind the chunks: the words' flags
    float* s_E = s_P + g.piece * kFprintChunk;                               // [piece + 1][33]: row 0 is the frame before the piece's first
    float* s_wc = s_E + (g.piece + 1) * kFprintMaxBands;                     // [32]
    float* s_ws = s_wc + 32;                                                 // [32]
    int* s_edges = reinterpret_cast<int*>(s_ws + 32);                        // [34], as columns of the transformed bins

    fmd_fprint_status* st = status + c;
    const unsigned long long frames0 = st->frames;
    const int fill = (int)st->fill;
    const unsigned long long s0 = frames0 / (unsigned long long)H;
    const int nsb = (int)(((long long)fill + n) / H);                        // 0 ... piece
    const unsigned long long s1 = s0 + (unsigned long long)nsb;
    const unsigned long long F0 = s0 >= (unsigned long long)R ? s0 - R + 1 : 0, F1 = s1 >= (unsigned long long)R ? s1 - R + 1 : 0;
    const int nfr = (int)(F1 - F0);                                          // frames of this piece, at most nsb
    const int nold = (int)(s0 < (unsigned long long)(R - 1) ? s0 : (unsigned long long)(R - 1));
    const unsigned long long g_lo = s0 - (unsigned long long)nold;           // LDS row j is sub-block g_lo + j; frame f's first row is f
    const int skip = F0 == 0 ? 1 : 0;                                        // frame 0 has no word
    const int nw = nfr > skip ? nfr - skip : 0;
    const int base = first_piece ? 0 : cnt_all[c];
    const float2* inrow = in + (size_t)c * (size_t)in_stride;
    float* ring = ring_all + (size_t)c * (size_t)(R - 1) * (size_t)ld;
    const float* mine = scratch + (size_t)rowbase[c] * (size_t)ld;           // this station's nsb new rows
    float* elast = elast_all + (size_t)c * kFprintMaxBands;

    if (nfr > 0) {
        if (tid < R) { s_wc[tid] = d_wc[tid]; s_ws[tid] = d_ws[tid]; }
        if (tid <= B) s_edges[tid] = d_edges[tid] - g.first;
        for (int i = tid; i < (nfr + 1) * kFprintMaxBands; i += kT) {
            const int f = i / kFprintMaxBands, b = i % kFprintMaxBands;
            s_E[i] = (f == 0 && !skip && b < B) ? elast[b] : 0.0f;
        }
        const int rows = nold + nsb;
        for (int ch0 = 0; ch0 < K - 2; ch0 += kFprintChunk) {
            const int cw = min(kFprintChunk, K - 2 - ch0), span = cw + 2;    // columns ch0 ... ch0 + cw + 1 are read, ch0 + 1 ... ch0 + cw come out
            __syncthreads();
            for (int i = tid; i < rows * span; i += kT) {
                const int j = i / span, x = i % span;
                const unsigned long long sb = g_lo + (unsigned long long)j;
                const float* src = sb < s0 ? ring + (size_t)(sb % (unsigned long long)(R - 1)) * (size_t)ld : mine + (size_t)(sb - s0) * (size_t)ld;
                s_S[j * kSpan + x] = float2{src[ch0 + x], src[Kp + ch0 + x]};
            }
            __syncthreads();
            for (int i = tid; i < nfr * span; i += kT) {
                const int f = i / span, x = i % span;
                const int k = g.first + ch0 + x;
                float re = 0.0f, im = 0.0f;
                for (int j = 0; j < R; j++) {
                    const int q = (k * j) & (R - 1);
                    const float2 s = s_S[(f + j) * kSpan + x];
                    const float wc = s_wc[q], ws = s_ws[q];
                    re = fmaf(s.x, wc, re); re = fmaf(s.y, ws, re);
                    im = fmaf(s.y, wc, im); im = fmaf(-s.x, ws, im);
                }
                s_X[f * kSpan + x] = float2{re, im};
            }
            __syncthreads();
            for (int i = tid; i < nfr * cw; i += kT) {
                const int f = i / cw, x = 1 + i % cw;
                const float2 a = s_X[f * kSpan + x - 1], m = s_X[f * kSpan + x], b = s_X[f * kSpan + x + 1];
                const float xr = fmaf(-0.25f, a.x + b.x, 0.5f * m.x), xi = fmaf(-0.25f, a.y + b.y, 0.5f * m.y);
                s_P[f * kFprintChunk + x - 1] = fmaf(xr, xr, xi * xi);
            }
            __syncthreads();
            for (int i = tid; i < nfr * B; i += kT) {
                const int f = i / B, b = i % B;
                const int k0 = max(s_edges[b], ch0 + 1), k1 = min(s_edges[b + 1], ch0 + cw + 1);
                float e = s_E[(f + 1) * kFprintMaxBands + b];
                for (int k = k0; k < k1; k++) e = e + s_P[f * kFprintChunk + k - ch0 - 1];
                s_E[(f + 1) * kFprintMaxBands + b] = e;
            }
        }
        __syncthreads();
        int* s_bad = reinterpret_cast<int*>(s_P);
        if (tid < nfr) {
            const int f = tid;
            int bad = 0;
            if (f >= skip) {
                const float* e1 = s_E + (f + 1) * kFprintMaxBands;
                const float* e0 = s_E + f * kFprintMaxBands;
                uint32_t w = 0;
                for (int b = 0; b < B - 1; b++) {
                    const float d0 = e1[b] - e1[b + 1], d1 = e0[b] - e0[b + 1];
                    const float d = d0 - d1;
                    if (d > 0.0f) w |= 1u << (31 - b);
                }
                for (int b = 0; b < B; b++) bad |= (fp_nonfinite(e1[b]) || fp_nonfinite(e0[b])) ? 1 : 0;
                out[(size_t)c * (size_t)out_stride + (size_t)(base + f - skip)] = w;
            }
            s_bad[f] = bad;
        }
        if (energy) {
            for (int i = tid; i < nfr * B; i += kT) {
                const int f = i / B, b = i % B;
                if (f >= skip) {
                    const float e = s_E[(f + 1) * kFprintMaxBands + b];
                    energy[(size_t)c * (size_t)energy_stride + (size_t)(base + f - skip) * (size_t)B + (size_t)b] = e != e ? __uint_as_float(0x7fc00000u) : e;
                }
            }
        }
        if (tid < B) elast[tid] = s_E[nfr * kFprintMaxBands + tid];
    }
    __syncthreads();                                                         // every read of the ring is done

    // ---- what the next call needs: the newest R - 1 spectra, the unconsumed samples, the record
    {
        const unsigned long long from = (s1 > (unsigned long long)(R - 1) && s1 - (R - 1) > s0) ? s1 - (R - 1) : s0;
        const int rows = (int)(s1 - from);
        for (int i = tid; i < rows * ld; i += kT) {
            const int j = i / ld, x = i % ld;
            const unsigned long long sb = from + (unsigned long long)j;
            ring[(size_t)(sb % (unsigned long long)(R - 1)) * (size_t)ld + x] = mine[(size_t)(sb - s0) * (size_t)ld + x];
        }
    }
    float* carry = carry_all + (size_t)c * (size_t)H;
    const int newfill = (int)((long long)fill + n - (long long)nsb * H);     // 0 ... H - 1
    if (nsb == 0) {
        for (int i = tid; i < (int)n; i += kT) { const float2 v = inrow[i]; carry[fill + i] = 0.5f * (v.x + v.y); }
    } else {
        for (int i = tid; i < newfill; i += kT) { const float2 v = inrow[n - newfill + i]; carry[i] = 0.5f * (v.x + v.y); }
    }
    if (tid == 0) {
        int bad = 0;
        if (nfr > 0) {
            const int* s_bad = reinterpret_cast<const int*>(s_P);
            for (int f = 0; f < nfr; f++) bad += s_bad[f];
        }
        st->frames = frames0 + (unsigned long long)n;
        st->prints += (unsigned long long)nw;
        st->nonfinite += (unsigned long long)bad;
        st->fill = (unsigned)newfill;
        cnt_all[c] = base + nw;
        if (last_piece && nprints) nprints[c] = base + nw;
    }
}

// stations c0 ... as after create
__global__ __launch_bounds__(64) void k_fprint_reset(int c0, int cn, fmd_fprint_status* __restrict__ status) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= cn) return;
    fmd_fprint_status z{};
    status[c0 + i] = z;
}

}  // namespace

struct fmd_fprint_s {
    fmd_fprint_config cfg{};
    FprintLayout lay{};
    FprintDev dev{};
    fmd_fprint_status* d_status = nullptr;   // [C]
    float* d_carry = nullptr;                // [C][H]: the open sub-block's mono samples
    float* d_ring = nullptr;                 // [C][R - 1][2 Kp]: the kept spectra; sub-block s lies in slot s mod (R - 1)
    float* d_elast = nullptr;                // [C][33]: E of the last frame
    float* d_scratch = nullptr;              // [C * piece][2 Kp]: a piece's new spectra
    int* d_rowbase = nullptr;                // [C + 1]
    int* d_cnt = nullptr;                    // [C]: the words of the call so far
    float* d_img = nullptr;                  // [H][2 Kp]: bc | bs, zero in the padding
    float* d_wc = nullptr;                   // [32]
    float* d_ws = nullptr;                   // [32]
    int* d_edges = nullptr;                  // [34]
    fmd::CallOrder order;                    // behind the previous call's work, for callers that change streams between calls
    std::string err;
};

template <typename... A>
static int fpr_fail(fmd_fprint h, int code, const char* fmt, A... args) { return fmd::fail(h ? h->err : fmd::fprint_global_error(), code, fmt, args...); }

extern "C" {

int fmd_fprint_create(const fmd_fprint_config* cfg, fmd_fprint* out) {
    if (!cfg || !out) return fpr_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    std::string why;
    FprintLayout L;
    if (fmd::fprint_check(cfg, &why) != FMD_OK || fmd::fprint_layout(cfg, &L, &why) != FMD_OK) return fpr_fail(nullptr, FMD_ERR_ARG, "%s", why.c_str());
    if ((long long)cfg->n_channels * L.piece > (1LL << 30)) return fpr_fail(nullptr, FMD_ERR_ARG, "n_channels * %d rows a piece above 2^30", L.piece);
    if (fmd_device_count() <= 0) return fpr_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return fpr_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_fprint h = new fmd_fprint_s();
    h->cfg = *cfg;
    h->lay = L;
    h->dev = FprintDev{cfg->hop, cfg->n_sub, cfg->n_bands, L.K, L.Kp, L.first_bin, L.piece};
    const size_t H = (size_t)cfg->hop, C = (size_t)cfg->n_channels, K = (size_t)L.K, ld = 2 * (size_t)L.Kp;
    std::vector<float> bc(H * K), bs(H * K), wc(32, 0.0f), ws(32, 0.0f), img(H * ld, 0.0f);
    std::vector<int> edges(kFprintMaxBands + 1, 0);
    if (fmd_fprint_design(cfg, bc.data(), bs.data(), wc.data(), ws.data(), edges.data(), nullptr) != FMD_OK) { delete h; return FMD_ERR_ARG; }
    for (size_t n = 0; n < H; n++)
        for (size_t k = 0; k < K; k++) { img[n * ld + k] = bc[n * K + k]; img[n * ld + (size_t)L.Kp + k] = bs[n * K + k]; }
    bool ok = h->order.init(dev);
    ok = ok && hipMalloc(&h->d_status, sizeof(fmd_fprint_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&h->d_carry, sizeof(float) * H * C) == hipSuccess;
    ok = ok && hipMalloc(&h->d_ring, sizeof(float) * C * (size_t)(cfg->n_sub - 1) * ld) == hipSuccess;
    ok = ok && hipMalloc(&h->d_elast, sizeof(float) * C * kFprintMaxBands) == hipSuccess;
    ok = ok && hipMalloc(&h->d_scratch, sizeof(float) * C * (size_t)L.piece * ld) == hipSuccess;
    ok = ok && hipMalloc(&h->d_rowbase, sizeof(int) * (C + 1)) == hipSuccess;
    ok = ok && hipMalloc(&h->d_cnt, sizeof(int) * C) == hipSuccess;
    ok = ok && hipMalloc(&h->d_img, sizeof(float) * img.size()) == hipSuccess;
    ok = ok && hipMalloc(&h->d_wc, sizeof(float) * 32) == hipSuccess;
    ok = ok && hipMalloc(&h->d_ws, sizeof(float) * 32) == hipSuccess;
    ok = ok && hipMalloc(&h->d_edges, sizeof(int) * edges.size()) == hipSuccess;
    ok = ok && hipMemcpy(h->d_img, img.data(), sizeof(float) * img.size(), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(h->d_wc, wc.data(), sizeof(float) * 32, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(h->d_ws, ws.data(), sizeof(float) * 32, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(h->d_edges, edges.data(), sizeof(int) * edges.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok || fmd_fprint_reset(h, -1) != FMD_OK) {
        (void)hipGetLastError();
        fmd_fprint_destroy(h);
        return fpr_fail(nullptr, FMD_ERR_DEVICE, "device allocation of %lld bytes failed", fmd::fprint_bytes(cfg, L, cfg->n_channels));
    }
    *out = h;
    return FMD_OK;
}

int fmd_fprint_destroy(fmd_fprint h) {
    if (!h) return FMD_ERR_ARG;
    (void)h->order.quiesce();
    for (void* p : {(void*)h->d_status, (void*)h->d_carry, (void*)h->d_ring, (void*)h->d_elast, (void*)h->d_scratch, (void*)h->d_rowbase, (void*)h->d_cnt, (void*)h->d_img,
                    (void*)h->d_wc, (void*)h->d_ws, (void*)h->d_edges})
        if (p) (void)hipFree(p);
    delete h;
    return FMD_OK;
}

int fmd_fprint_reset(fmd_fprint h, int channel) {
    if (!h) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, h->cfg.n_channels, &c0, &cn)) return fpr_fail(h, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, h->cfg.n_channels);
    if (!h->order.quiesce()) return fpr_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_fprint_reset, dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, nullptr, c0, cn, h->d_status);
    if (const char* e = fmd::control_end("k_fprint_reset launch failed")) return fpr_fail(h, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_fprint_process_f32_dev(fmd_fprint h, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint32_t* d_out, long long out_stride,
                               int* d_nprints, float* d_energy, long long energy_stride, void* stream) {
    if (!h) return FMD_ERR_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return fpr_fail(h, FMD_ERR_ARG, "null input, or input not aligned to 8 bytes");
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 4 != 0) return fpr_fail(h, FMD_ERR_ARG, "null output, or output not aligned to 4 bytes");
    if (reinterpret_cast<uintptr_t>(d_energy) % 4 != 0) return fpr_fail(h, FMD_ERR_ARG, "energies not aligned to 4 bytes");
    if (n < 0 || n > in_stride || n > h->cfg.max_input_frames)
        return fpr_fail(h, FMD_ERR_ARG, "n %lld outside [0, in_stride %lld] or above max_input_frames %lld", n, in_stride, h->cfg.max_input_frames);
    const long long need = fmd_fprint_max_prints(h->cfg.hop, n);
    if (out_stride < need) return fpr_fail(h, FMD_ERR_ARG, "out_stride %lld below the %lld words the call may write", out_stride, need);
    if (d_energy && energy_stride < need * h->cfg.n_bands)
        return fpr_fail(h, FMD_ERR_ARG, "energy_stride %lld below the %lld floats the call may write", energy_stride, need * h->cfg.n_bands);
    if (n == 0 && !d_nprints) return FMD_OK;                                 // nothing of any station changes and there is no count to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* e = h->order.begin(s)) return fpr_fail(h, FMD_ERR_DEVICE, "%s", e);
    const int C = h->cfg.n_channels, H = h->cfg.hop;
    const size_t lds = sizeof(float) * (size_t)h->lay.lds_floats;
    const int ntiles = 2 * h->lay.Kp / kFprintTile, per_wg = (kT / 64) * kCT;
    // a call longer than the scratch holds goes piece by piece: the same words, by the rule that nothing depends on the split
    long long at = 0;
    do {
        const long long np = n - at < h->lay.piece_frames ? n - at : h->lay.piece_frames;
        const float2* in = reinterpret_cast<const float2*>(d_in) + at;
        const int first = at == 0, last = at + np == n;
        hipLaunchKernelGGL(k_fprint_map, dim3(1), dim3(fmd::rowmap::kThreads), 0, s, C, np, d_active, h->d_status, H, h->d_rowbase);
        const long long rows_max = (long long)C * ((np + H - 1) / H);        // at most C * piece
        if (rows_max > 0)
            hipLaunchKernelGGL(k_fprint_sub, dim3((unsigned)((rows_max + kRT * kFprintTile - 1) / (kRT * kFprintTile)), (unsigned)((ntiles + per_wg - 1) / per_wg)), dim3(kT),
                               0, s, in, in_stride, C, h->dev, h->d_rowbase, h->d_status, h->d_carry, h->d_img, h->d_scratch);
        hipLaunchKernelGGL(k_fprint_frame, dim3((unsigned)C), dim3(kT), lds, s, in, in_stride, np, d_active, h->dev, h->d_rowbase, h->d_scratch, h->d_wc, h->d_ws,
                           h->d_edges, h->d_status, h->d_carry, h->d_ring, h->d_elast, h->d_cnt, first, last, d_out, out_stride, d_nprints, d_energy, energy_stride);
        if (hipGetLastError() != hipSuccess) return fpr_fail(h, FMD_ERR_DEVICE, "k_fprint launch failed");
        at += np;
    } while (at < n);
    if (const char* e = h->order.end(s)) return fpr_fail(h, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_fprint_get_status(fmd_fprint h, fmd_fprint_status* out) {
    if (!h || !out) return fpr_fail(h, FMD_ERR_ARG, "null object or output");
    if (!h->order.quiesce()) return fpr_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, h->d_status, sizeof(fmd_fprint_status) * (size_t)h->cfg.n_channels, hipMemcpyDeviceToHost) != hipSuccess)
        return fpr_fail(h, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_fprint_status_dev(fmd_fprint h, const fmd_fprint_status** d_status) {
    if (!h || !d_status) return fpr_fail(h, FMD_ERR_ARG, "null object or output");
    *d_status = h->d_status;
    return FMD_OK;
}

const char* fmd_fprint_last_error(fmd_fprint h) { return h ? h->err.c_str() : fmd::fprint_global_error().c_str(); }

}  // extern "C"
