// FLAC audio encoder, device side (include/fmdemod.h, "FLAC audio encoder").
//
// NOT in the reference.  Lossless recordings of the station audio [C][in_stride][2] f32 that the mixer and the monitors read, read in
// place: per station a fixed-blocksize FLAC stream (RFC 9639, streamable subset) of frames of S audio frames, written byte-packed to a
// caller-owned device array as the blocks complete.
//
// One workgroup of four wavefronts per station walks that station's completed blocks in order, so a frame's byte offset is a running sum
// inside the workgroup and no workgroup waits on another.  Per block the q words (qL | qR << 16) go to LDS, from the encoder's open block
// and from d_in, converted and counted where they are loaded.  Wavefront w then plans channel candidate w (L, R, M, Sd): lane l owns
// finest partition l of the 2^pmax (pmax = 6 for a whole block: n / 64 consecutive samples), sums |r| of the five fixed predictors over
// it, the wavefront picks the order, and for that order the lane sums u >> k for the 15 Rice parameters.  Coarser partitions are pair
// sums up a six-level tree of lane shuffles; each level's cost is a wave sum.  After a barrier every thread picks the channel assignment
// from the four totals; wavefronts 0 and 1 write the two subframes into a zeroed LDS image of the frame (bit positions by a wave prefix
// sum of the lanes' lengths, words OR-ed in with LDS atomics, most significant bit first), a lane of wavefront 2 writes the frame
// header and its CRC-8.  Wavefront 0 takes the CRC-16: a lane each over a 64th of the bytes, combined with x^(8 m) mod P factors from
// the host's table, the CRC being linear.  The image leaves with ordinary 4-byte stores, byte stores at a frame's unaligned ends.  The
// short frame of a flush runs the same device functions in a kernel of its own; with an odd length one lane per candidate does the
// work.  Every LDS index is bounded by the validated n and fmd_flac_frame_bound, every global index by n, the strides and that bound.
// No global atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fmd_flac_design.h"
#include "fmd_side.h"
#include "fmdemod.h"
#include "fmdemod_flac_debug.h"

namespace {

constexpr int kT = 256;              // threads per workgroup: four wavefronts, one per channel candidate
constexpr int kPowSlack = 128;       // entries of the x^(8 m) table past the frame bound (a lane's factor index is below bytes + 64)

static_assert(sizeof(fmd_flac_status) == 80 && offsetof(fmd_flac_status, blocks) == 8 && offsetof(fmd_flac_status, stream_samples) == 16 &&
              offsetof(fmd_flac_status, stream_bytes) == 24 && offsetof(fmd_flac_status, clipped) == 32 && offsetof(fmd_flac_status, nonfinite) == 48 &&
              offsetof(fmd_flac_status, streams) == 56 && offsetof(fmd_flac_status, frame_number) == 60 && offsetof(fmd_flac_status, min_frame_bytes) == 64 &&
              offsetof(fmd_flac_status, max_frame_bytes) == 68 && offsetof(fmd_flac_status, fill) == 72 && offsetof(fmd_flac_status, wrapped) == 76,
              "fmd_flac_status layout");

typedef float fl_f2 __attribute__((ext_vector_type(2)));

// what the four wavefronts hand each other
struct FlShared {
    int k[4][64];                    // candidate, partition of the chosen order: the Rice parameter
    unsigned cand[4][4];             // candidate: type (0 CONSTANT, 1 VERBATIM, 2 FIXED), predictor order, partition order, bits
    unsigned short crc[256];         // the CRC-16 of each single byte
    unsigned cnt[3];                 // this call's clipped L, clipped R, non-finite samples
};

// the stream's counters as the workgroup carries them through a call (the same in every thread)
struct FlStream {
    unsigned long long blocks, samples, bytes;
    unsigned streams, number, minb, maxb, wrapped;
};

// the contract's sample: q, and whether it was clamped or not finite
__device__ __forceinline__ int fl_q(float x, unsigned& clip, unsigned& nonf) {
    const float t = x * (32767.0f * 0.95f);
    if (!(fabsf(t) <= 3.402823466e38f)) { nonf++; return 0; }
    if (t >= 32768.0f) { clip++; return 32767; }                             // (int)t > 32767
    if (t <= -32769.0f) { clip++; return -32768; }                           // (int)t < -32768
    return (int)t;
}

__device__ __forceinline__ uint32_t fl_pack(fl_f2 v, unsigned& cl, unsigned& cr, unsigned& nf) {
    const int l = fl_q(v.x, cl, nf), r = fl_q(v.y, cr, nf);
    return ((uint32_t)l & 0xffffu) | ((uint32_t)r << 16);
}

// sample i of candidate cand (0 L, 1 R, 2 M, 3 Sd); cand is the same in every lane
__device__ __forceinline__ int fl_x(const uint32_t* s_q, int cand, int i) {
    const uint32_t w = s_q[i];
    const int l = (int)(short)(w & 0xffffu), r = (int)w >> 16;
    return cand == 0 ? l : cand == 1 ? r : cand == 2 ? (l + r) >> 1 : l - r;
}

__device__ __forceinline__ unsigned long long fl_shfl64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long fl_wave_sum64(unsigned long long v, int lane) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += fl_shfl64(v, lane ^ d);
    return v;
}

// the order-o fixed predictor's residual; x1 ... x4 are the samples before x (|x| < 2^17: 24-bit multiplies)
__device__ __forceinline__ int fl_res(int o, int x, int x1, int x2, int x3, int x4) {
    const int c1 = o, c2 = o < 2 ? 0 : o == 2 ? -1 : o == 3 ? -3 : -6, c3 = o < 3 ? 0 : o == 3 ? 1 : 4, c4 = o == 4 ? -1 : 0;
    return x - (__mul24(c1, x1) + __mul24(c2, x2) + __mul24(c3, x3) + __mul24(c4, x4));
}

__device__ __forceinline__ unsigned fl_zigzag(int r) { return r >= 0 ? 2u * (unsigned)r : 2u * (unsigned)(-r) - 1u; }

// len <= 32 bits of v at bit `pos` of the image (most significant bit first; the image's words hold their bytes big-endian)
__device__ __forceinline__ void fl_put(uint32_t* img, int img_words, unsigned pos, uint32_t v, int len) {
    const int wi = (int)(pos >> 5), sh = 32 - (int)(pos & 31u) - len;
    if (len <= 0 || wi + 1 >= img_words) return;                             // (never: the frame is within its bound)
    if (sh >= 0) atomicOr(&img[wi], v << sh);
    else {
        atomicOr(&img[wi], v >> (-sh));
        atomicOr(&img[wi + 1], v << (32 + sh));
    }
}

__device__ __forceinline__ unsigned fl_byte(const uint32_t* img, int i) { return (img[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }

__device__ __forceinline__ int fl_block_code(int n) {
    if (n == 192) return 1;
    if (n == 576) return 2;
    if (n == 1152) return 3;
    if (n == 2304) return 4;
    if (n == 4608) return 5;
    if (n >= 256 && (n & (n - 1)) == 0) return 8 + (31 - __clz(n)) - 8;      // 256 << (code - 8); n <= 4608
    return n <= 256 ? 6 : 7;
}

__device__ __forceinline__ int fl_number_bytes(unsigned v) { return v < 0x80u ? 1 : v < 0x800u ? 2 : v < 0x10000u ? 3 : v < 0x200000u ? 4 : v < 0x4000000u ? 5 : 6; }

__device__ __forceinline__ int fl_header_bytes(int n, int sr_code, unsigned number) {
    const int bc = fl_block_code(n);
    return 4 + fl_number_bytes(number) + (bc == 6 ? 1 : bc == 7 ? 2 : 0) + (sr_code == 13 ? 2 : 0) + 1;
}

// the largest p <= 6 with 2^p dividing n
__device__ __forceinline__ int fl_pmax(int n) {
    const int tz = __ffs(n) - 1;
    return tz < 6 ? tz : 6;
}

// one wavefront plans candidate `cand` of n samples of b bits: s.cand[cand] and s.k[cand]
__device__ __forceinline__ void fl_plan(const uint32_t* s_q, FlShared& s, int cand, int n, int b, int lane) {
    const int pmax = fl_pmax(n), m = n >> pmax;
    const bool own = lane < (1 << pmax);
    const int a0 = own ? lane * m : 0, a1 = own ? a0 + m : 0;
    const int omax = n - 1 < 4 ? n - 1 : 4;
    // the five predictors' |r| sums over i >= omax, and whether every sample is the first
    const int first = fl_x(s_q, cand, 0);
    unsigned long long a[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    bool differs = false;
    {
        int x1 = a0 >= 1 ? fl_x(s_q, cand, a0 - 1) : 0, x2 = a0 >= 2 ? fl_x(s_q, cand, a0 - 2) : 0;
        int x3 = a0 >= 3 ? fl_x(s_q, cand, a0 - 3) : 0, x4 = a0 >= 4 ? fl_x(s_q, cand, a0 - 4) : 0;
        for (int i = a0; i < a1; i++) {                                      // (i < n)
            const int x = fl_x(s_q, cand, i);
            differs |= x != first;
            if (i >= omax) {
#pragma unroll
                for (int o = 0; o < 5; o++) {
                    const int r = fl_res(o, x, x1, x2, x3, x4);
                    a[o] += (unsigned long long)(unsigned)(r < 0 ? -r : r);
                }
            }
            x4 = x3; x3 = x2; x2 = x1; x1 = x;
        }
    }
    if (!__any(differs)) {                                                   // (the same in every lane)
        if (lane == 0) { s.cand[cand][0] = 0u; s.cand[cand][1] = 0u; s.cand[cand][2] = 0u; s.cand[cand][3] = 8u + (unsigned)b; }
        return;
    }
    int o = 0;
    unsigned long long best_a = 0ull;
#pragma unroll
    for (int t = 0; t < 5; t++) {
        const unsigned long long v = fl_wave_sum64(a[t], lane);
        if (t <= omax && (t == 0 || v < best_a)) { best_a = v; o = t; }
    }
    // the chosen order's sums of u >> k over the lane's residuals (i >= o), 32-bit over at most 1024 samples at a time (u < 2^22)
    unsigned long long sum[15];
#pragma unroll
    for (int k = 0; k < 15; k++) sum[k] = 0ull;
    unsigned long long cnt = 0ull;
    {
        const int s0 = a0 > o ? a0 : o;
        for (int c0 = s0; c0 < a1; c0 += 1024) {
            const int c1 = c0 + 1024 < a1 ? c0 + 1024 : a1;
            unsigned acc[15];
#pragma unroll
            for (int k = 0; k < 15; k++) acc[k] = 0u;
            int x1 = c0 >= 1 ? fl_x(s_q, cand, c0 - 1) : 0, x2 = c0 >= 2 ? fl_x(s_q, cand, c0 - 2) : 0;
            int x3 = c0 >= 3 ? fl_x(s_q, cand, c0 - 3) : 0, x4 = c0 >= 4 ? fl_x(s_q, cand, c0 - 4) : 0;
            for (int i = c0; i < c1; i++) {
                const int x = fl_x(s_q, cand, i);
                const unsigned u = fl_zigzag(fl_res(o, x, x1, x2, x3, x4));
#pragma unroll
                for (int k = 0; k < 15; k++) acc[k] += u >> k;
                x4 = x3; x3 = x2; x2 = x1; x1 = x;
            }
#pragma unroll
            for (int k = 0; k < 15; k++) sum[k] += acc[k];
            cnt += (unsigned long long)(c1 - c0);
        }
    }
    // up the tree: at level p lanes 0 ... 2^p - 1 hold partition `lane`'s sums
    int kb[7] = {0, 0, 0, 0, 0, 0, 0};
    int pstar = 0;
    unsigned long long best = 0ull;
    bool have = false;
#pragma unroll
    for (int p = 6; p >= 0; p--) {
        if (p > pmax) continue;                                              // (uniform)
        int kmin = 0;
        unsigned long long bmin = cnt + sum[0];
#pragma unroll
        for (int k = 1; k < 15; k++) {
            const unsigned long long v = cnt * (unsigned long long)(k + 1) + sum[k];
            if (v < bmin) { bmin = v; kmin = k; }
        }
        kb[p] = kmin;
        const unsigned long long cost = 6ull + fl_wave_sum64(lane < (1 << p) ? 4ull + bmin : 0ull, lane);
        if ((p == 0 || (n >> p) > o) && (!have || cost <= best)) { best = cost; pstar = p; have = true; }   // ties go to the lower p
        if (p > 0) {
#pragma unroll
            for (int k = 0; k < 15; k++) sum[k] = fl_shfl64(sum[k], (2 * lane) & 63) + fl_shfl64(sum[k], (2 * lane + 1) & 63);
            cnt = fl_shfl64(cnt, (2 * lane) & 63) + fl_shfl64(cnt, (2 * lane + 1) & 63);
        }
    }
    int ksel = kb[0];
#pragma unroll
    for (int p = 1; p < 7; p++)
        if (pstar == p) ksel = kb[p];
    const unsigned long long fixed = 8ull + (unsigned long long)(o * b) + best, verbatim = 8ull + (unsigned long long)n * (unsigned long long)b;
    const bool use = fixed < verbatim;
    if (use && lane < (1 << pstar)) s.k[cand][lane] = ksel;
    if (lane == 0) {
        s.cand[cand][0] = use ? 2u : 1u; s.cand[cand][1] = (unsigned)o; s.cand[cand][2] = (unsigned)pstar;
        s.cand[cand][3] = (unsigned)(use ? fixed : verbatim);
    }
}

// one wavefront writes candidate `cand`'s subframe from bit `start` on
__device__ __forceinline__ void fl_write_subframe(const uint32_t* s_q, uint32_t* img, int img_words, const FlShared& s, int cand, int n, int b, unsigned start, int lane) {
    const unsigned type = s.cand[cand][0];
    const uint32_t mask = (1u << b) - 1u;
    if (type == 0u) {
        if (lane == 0) fl_put(img, img_words, start + 8u, (uint32_t)fl_x(s_q, cand, 0) & mask, b);
        return;
    }
    if (type == 1u) {
        if (lane == 0) fl_put(img, img_words, start, 0x02u, 8);
        for (int i = lane; i < n; i += 64) fl_put(img, img_words, start + 8u + (unsigned)(i * b), (uint32_t)fl_x(s_q, cand, i) & mask, b);
        return;
    }
    const int o = (int)s.cand[cand][1], pstar = (int)s.cand[cand][2];
    if (lane == 0) {
        fl_put(img, img_words, start, (uint32_t)((8 | o) << 1), 8);
        for (int i = 0; i < o; i++) fl_put(img, img_words, start + 8u + (unsigned)(i * b), (uint32_t)fl_x(s_q, cand, i) & mask, b);
        fl_put(img, img_words, start + 8u + (unsigned)(o * b) + 2u, (uint32_t)pstar, 4);
    }
    const unsigned r0 = start + 8u + (unsigned)(o * b) + 6u;
    const int pmax = fl_pmax(n), m = n >> pmax;
    const bool own = lane < (1 << pmax);
    const int a0 = own ? lane * m : 0, a1 = own ? a0 + m : 0, s0 = a0 > o ? a0 : o;
    const int k = own ? s.k[cand][lane >> (pmax - pstar)] : 0;
    const bool head = own && (lane & ((1 << (pmax - pstar)) - 1)) == 0;      // the lane's samples begin a partition
    unsigned len = head ? 4u : 0u;
    {
        int x1 = s0 >= 1 ? fl_x(s_q, cand, s0 - 1) : 0, x2 = s0 >= 2 ? fl_x(s_q, cand, s0 - 2) : 0;
        int x3 = s0 >= 3 ? fl_x(s_q, cand, s0 - 3) : 0, x4 = s0 >= 4 ? fl_x(s_q, cand, s0 - 4) : 0;
        for (int i = s0; i < a1; i++) {
            const int x = fl_x(s_q, cand, i);
            len += (fl_zigzag(fl_res(o, x, x1, x2, x3, x4)) >> k) + 1u + (unsigned)k;
            x4 = x3; x3 = x2; x2 = x1; x1 = x;
        }
    }
    unsigned incl = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)incl, d);
        if (lane >= d) incl += t;
    }
    unsigned pos = r0 + incl - len;
    if (head) { fl_put(img, img_words, pos, (uint32_t)k, 4); pos += 4u; }
    {
        int x1 = s0 >= 1 ? fl_x(s_q, cand, s0 - 1) : 0, x2 = s0 >= 2 ? fl_x(s_q, cand, s0 - 2) : 0;
        int x3 = s0 >= 3 ? fl_x(s_q, cand, s0 - 3) : 0, x4 = s0 >= 4 ? fl_x(s_q, cand, s0 - 4) : 0;
        for (int i = s0; i < a1; i++) {
            const int x = fl_x(s_q, cand, i);
            const unsigned u = fl_zigzag(fl_res(o, x, x1, x2, x3, x4));
            pos += u >> k;                                                   // the zeros are there
            fl_put(img, img_words, pos, (1u << k) | (u & ((1u << k) - 1u)), k + 1);
            pos += (unsigned)k + 1u;
            x4 = x3; x3 = x2; x2 = x1; x1 = x;
        }
    }
}

__device__ __forceinline__ unsigned fl_gfmul(unsigned a, unsigned b) {      // a * b mod x^16 + x^15 + x^2 + 1
    unsigned r = 0u;
#pragma unroll
    for (int i = 15; i >= 0; i--) {
        r = (r << 1) ^ ((r & 0x8000u) ? 0x18005u : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r & 0xffffu;
}

// All kT threads: the frame of the n <= S samples in s_q, numbered `number`, into the zeroed image; returns its bytes.  A barrier
// stands in front of the first use of s_q and the image and behind the last write of the image.
__device__ __forceinline__ int fl_encode_frame(const uint32_t* s_q, uint32_t* img, int img_words, FlShared& s, int n, int fs, int sr_code, unsigned number,
                               const unsigned short* __restrict__ pow8) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __syncthreads();
    fl_plan(s_q, s, wave, n, wave == 3 ? 17 : 16, lane);
    __syncthreads();
    const unsigned bl = s.cand[0][3], br = s.cand[1][3], bm = s.cand[2][3], bs = s.cand[3][3];
    int mode = 0;                                                            // 0 (L, R), 1 (L, Sd), 2 (Sd, R), 3 (M, Sd): ties in that order
    unsigned tot = bl + br;
    if (bl + bs < tot) { tot = bl + bs; mode = 1; }
    if (bs + br < tot) { tot = bs + br; mode = 2; }
    if (bm + bs < tot) { tot = bm + bs; mode = 3; }
    const int c0 = mode == 2 ? 3 : mode == 3 ? 2 : 0, c1 = (mode == 1 || mode == 3) ? 3 : 1;
    const int hdr = fl_header_bytes(n, sr_code, number);
    const unsigned bits0 = s.cand[c0][3];
    const int nbytes = hdr + (int)((bits0 + s.cand[c1][3] + 7u) >> 3);
    if (wave < 2) {
        const int cw = wave == 0 ? c0 : c1;
        fl_write_subframe(s_q, img, img_words, s, cw, n, cw == 3 ? 17 : 16, 8u * (unsigned)hdr + (wave == 0 ? 0u : bits0), lane);
    } else if (tid == 128) {
        unsigned crc = 0u, at = 0u;
        auto byte = [&](unsigned v) {
            fl_put(img, img_words, at, v, 8);
            at += 8u;
            crc ^= v;
            for (int i = 0; i < 8; i++) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xffu : (crc << 1) & 0xffu;
        };
        const int bc = fl_block_code(n);
        const unsigned code = mode == 0 ? 1u : mode == 1 ? 8u : mode == 2 ? 9u : 10u;
        byte(0xffu); byte(0xf8u);
        byte((unsigned)((bc << 4) | sr_code));
        byte((code << 4) | (4u << 1));
        const int extra = fl_number_bytes(number) - 1;
        if (extra == 0) byte(number);
        else {
            byte(((0xff00u >> (extra + 1)) & 0xffu) | (number >> (6 * extra)));
            for (int i = 1; i <= extra; i++) byte(0x80u | ((number >> (6 * (extra - i))) & 0x3fu));
        }
        if (bc == 6) byte((unsigned)(n - 1));
        if (bc == 7) { byte((unsigned)(n - 1) >> 8); byte((unsigned)(n - 1) & 255u); }
        if (sr_code == 13) { byte((unsigned)fs >> 8); byte((unsigned)fs & 255u); }
        byte(crc);
    }
    __syncthreads();
    if (wave == 0) {
        // lane l takes bytes [nbytes - (64 - l) c, nbytes - (63 - l) c): zero bytes in front of a message do not change its CRC
        const int c = (nbytes + 63) >> 6;
        const int e1 = nbytes - (63 - lane) * c, e0 = e1 - c;
        unsigned crc = 0u;
        for (int i = e0 < 0 ? 0 : e0; i < e1; i++) crc = ((crc << 8) & 0xffffu) ^ s.crc[(crc >> 8) ^ fl_byte(img, i)];   // (i < nbytes)
        crc = fl_gfmul(crc, pow8[(63 - lane) * c]);                          // ((63 - lane) c < nbytes + 63)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) crc ^= (unsigned)__shfl_xor((int)crc, d);
        if (lane == 0) fl_put(img, img_words, 8u * (unsigned)nbytes, crc, 16);
    }
    __syncthreads();
    return nbytes + 2;
}

// the image's first nbytes bytes to dst: whole aligned words where dst allows, single bytes at the ends
__device__ __forceinline__ void fl_copy_out(const uint32_t* img, int nbytes, uint8_t* dst) {
    const int tid = threadIdx.x;
    const int d0 = (int)(reinterpret_cast<uintptr_t>(dst) & 3u);
    const int head = d0 == 0 ? 0 : (4 - d0 < nbytes ? 4 - d0 : nbytes);
    if (tid < head) dst[tid] = (uint8_t)fl_byte(img, tid);
    const int body = (nbytes - head) >> 2;
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    for (int j = tid; j < body; j += kT) {
        const int at = head + 4 * j, sh = 8 * (at & 3);
        const uint32_t w0 = img[at >> 2], w1 = img[(at >> 2) + 1];           // (at + 3 < nbytes: both words are the image's)
        const uint32_t v = sh == 0 ? w0 : (w0 << sh) | (w1 >> (32 - sh));
        dw[j] = __builtin_bswap32(v);
    }
    const int tail = head + 4 * body;
    if (tid < nbytes - tail) dst[tail + tid] = (uint8_t)fl_byte(img, tail + tid);
}

// the stream's counters behind a written frame of n samples and `bytes` bytes; true where the stream ended behind it by itself
__device__ __forceinline__ bool fl_account(FlStream& f, int n, int bytes) {
    f.blocks++;
    f.samples += (unsigned long long)n;
    f.bytes += (unsigned long long)bytes;
    if (f.minb == 0u || (unsigned)bytes < f.minb) f.minb = (unsigned)bytes;
    if ((unsigned)bytes > f.maxb) f.maxb = (unsigned)bytes;
    if (f.number == 0x7fffffffu) {                                           // the number would reach 2^31: a new stream
        f.streams++; f.number = 0u; f.samples = 0ull; f.bytes = 0ull; f.minb = 0u; f.maxb = 0u; f.wrapped = 1u;
        return true;
    }
    f.number++;
    return false;
}

__device__ __forceinline__ FlStream fl_load(const fmd_flac_status* st) {
    FlStream f;
    f.blocks = st->blocks; f.samples = st->stream_samples; f.bytes = st->stream_bytes;
    f.streams = st->streams; f.number = st->frame_number; f.minb = st->min_frame_bytes; f.maxb = st->max_frame_bytes; f.wrapped = st->wrapped;
    return f;
}

__device__ __forceinline__ void fl_store(fmd_flac_status* st, const FlStream& f) {
    st->blocks = f.blocks; st->stream_samples = f.samples; st->stream_bytes = f.bytes;
    st->streams = f.streams; st->frame_number = f.number; st->min_frame_bytes = f.minb; st->max_frame_bytes = f.maxb; st->wrapped = f.wrapped;
}

__device__ __forceinline__ void fl_tables(FlShared& s, const unsigned short* __restrict__ crc_tab) {
    const int tid = threadIdx.x;
    s.crc[tid] = crc_tab[tid];                                               // (kT == 256)
    if (tid < 3) s.cnt[tid] = 0u;
    __syncthreads();
}
static_assert(kT == 256, "fl_tables: a thread per table entry");

// in [C][in_stride] frames (L, R); status [C]; open [C][S] words; out: station c's frames from byte c * out_stride on.
// Dynamic LDS: S words of q, then img_words words of the frame's image.
__global__ __launch_bounds__(kT) void k_flac(const fl_f2* __restrict__ in, long long in_stride, int n, const uint8_t* __restrict__ active, int S, int fs, int sr_code,
                                             int img_words, fmd_flac_status* __restrict__ status, uint32_t* __restrict__ open,
                                             const unsigned short* __restrict__ crc_tab, uint8_t* __restrict__ out, long long out_stride,
                                             int* __restrict__ nbytes_out, int* __restrict__ nframes_out) {
    extern __shared__ uint32_t s_dyn[];
    __shared__ FlShared s;
    uint32_t* s_q = s_dyn;
    uint32_t* img = s_dyn + S;
    const int tid = threadIdx.x, c = blockIdx.x;
    if (active && active[c] == 0) {                                          // a skipped station (the same in every thread)
        if (tid == 0) {
            if (nbytes_out) nbytes_out[c] = 0;
            if (nframes_out) nframes_out[c] = 0;
        }
        return;
    }
    fl_tables(s, crc_tab);
    fmd_flac_status* stp = status + c;
    const int fill = (int)stp->fill;                                         // < S
    FlStream f = fl_load(stp);
    const int nf = (int)(((long long)fill + n) / S);                         // (n <= 2^30)
    const fl_f2* row = in + (size_t)c * (size_t)in_stride;
    uint32_t* opn = open + (size_t)c * (size_t)S;
    uint8_t* orow = out + (size_t)c * (size_t)out_stride;
    unsigned cl = 0u, cr = 0u, nonf = 0u;
    long long off = 0;                                                       // bytes written so far
    for (int j = 0; j < nf; j++) {
        const long long g0 = (long long)j * S - fill;                        // the block's first sample in the call's input
        __syncthreads();                                                     // the frame before has left the image
        for (int t = tid; t < S; t += kT) {
            const long long g = g0 + t;                                      // (g < n: the block completes within the call)
            s_q[t] = g < 0 ? opn[t] : fl_pack(__builtin_nontemporal_load(row + g), cl, cr, nonf);   // (g < 0: t < fill)
        }
        for (int t = tid; t < img_words; t += kT) img[t] = 0u;
        const int bytes = fl_encode_frame(s_q, img, img_words, s, S, fs, sr_code, f.number, crc_tab + 256);
        if (off + bytes <= out_stride) fl_copy_out(img, bytes, orow + off);  // (always: a frame is within fmd_flac_frame_bound)
        off += bytes;
        fl_account(f, S, bytes);
    }
    // what is left goes to the open block
    const int rem = (int)((long long)fill + n - (long long)nf * S);          // < S
    const long long r0 = nf > 0 ? (long long)nf * S - fill : 0;              // the first left-over sample in the input
    const int o0 = nf > 0 ? 0 : fill;                                        // and its place in the open block
    for (long long g = r0 + tid; g < n; g += kT) opn[o0 + (int)(g - r0)] = fl_pack(__builtin_nontemporal_load(row + g), cl, cr, nonf);   // (o0 + n - r0 = rem < S)
    if (cl) atomicAdd(&s.cnt[0], cl);
    if (cr) atomicAdd(&s.cnt[1], cr);
    if (nonf) atomicAdd(&s.cnt[2], nonf);
    __syncthreads();
    if (tid == 0) {
        fl_store(stp, f);
        stp->frames += (unsigned long long)n;
        stp->clipped[0] += s.cnt[0]; stp->clipped[1] += s.cnt[1]; stp->nonfinite += s.cnt[2];
        stp->fill = (unsigned)rem;
        if (nbytes_out) nbytes_out[c] = (int)off;
        if (nframes_out) nframes_out[c] = nf;
    }
}

// stations c0 ... c0 + cn - 1: the stream ended, behind a short last frame where the open block holds samples
__global__ __launch_bounds__(kT) void k_flac_flush(int c0, int S, int fs, int sr_code, int img_words, fmd_flac_status* __restrict__ status,
                                                   const uint32_t* __restrict__ open, const unsigned short* __restrict__ crc_tab, uint8_t* __restrict__ out,
                                                   long long out_stride, int* __restrict__ nbytes_out, int* __restrict__ nframes_out) {
    extern __shared__ uint32_t s_dyn[];
    __shared__ FlShared s;
    uint32_t* s_q = s_dyn;
    uint32_t* img = s_dyn + S;
    const int tid = threadIdx.x, c = c0 + blockIdx.x;
    fl_tables(s, crc_tab);
    fmd_flac_status* stp = status + c;
    const int fill = (int)stp->fill;                                         // < S (the same in every thread)
    FlStream f = fl_load(stp);
    int bytes = 0;
    bool wrapped = false;
    if (fill > 0) {
        const uint32_t* opn = open + (size_t)c * (size_t)S;
        for (int t = tid; t < fill; t += kT) s_q[t] = opn[t];
        for (int t = tid; t < img_words; t += kT) img[t] = 0u;
        bytes = fl_encode_frame(s_q, img, img_words, s, fill, fs, sr_code, f.number, crc_tab + 256);
        if (bytes <= out_stride) fl_copy_out(img, bytes, out + (size_t)c * (size_t)out_stride);
        wrapped = fl_account(f, fill, bytes);
    }
    if (!wrapped) { f.streams++; f.number = 0u; f.samples = 0ull; f.bytes = 0ull; f.minb = 0u; f.maxb = 0u; }
    if (tid == 0) {
        fl_store(stp, f);
        stp->fill = 0u;
        if (nbytes_out) nbytes_out[c] = bytes;
        if (nframes_out) nframes_out[c] = fill > 0 ? 1 : 0;
    }
}

// stations c0 ... c0 + cn - 1 as after create
__global__ __launch_bounds__(64) void k_flac_reset(int c0, int cn, fmd_flac_status* __restrict__ status) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= cn) return;
    uint4* w = reinterpret_cast<uint4*>(status + c0 + i);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(fmd_flac_status) / 16); k++) w[k] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

struct fmd_flac_s {
    int C = 0, S = 0, fs = 0, sr_code = 0, img_words = 0;
    long long max_in = 0;
    fmd_flac_status* d_status = nullptr;     // [C]
    uint32_t* d_open = nullptr;              // [C][S]: each station's open block, (qL | qR << 16)
    unsigned short* d_crc = nullptr;         // fmd::flac_crc16_tables
    fmd::CallOrder order;                    // behind the previous call's work, for callers that change streams between calls
    std::string err;
    size_t lds() const { return sizeof(uint32_t) * (size_t)(S + img_words); }
};

template <typename... A>
static int fl_fail(fmd_flac e, int code, const char* fmt, A... args) { return fmd::fail(e ? e->err : fmd::flac_global_error(), code, fmt, args...); }

extern "C" {

int fmd_flac_create(const fmd_flac_config* cfg, fmd_flac* out) {
    if (!cfg || !out) return fl_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    if (cfg->n_channels <= 0 || cfg->max_input_frames <= 0 || cfg->max_input_frames > (1LL << 30))
        return fl_fail(nullptr, FMD_ERR_ARG, "n_channels %d is not positive or max_input_frames %lld outside (0, 2^30]", cfg->n_channels, cfg->max_input_frames);
    const int S = fmd::flac_block_frames(cfg->block_frames);
    if (S == 0) return fl_fail(nullptr, FMD_ERR_ARG, "block_frames %d is neither 0 nor a multiple of 64 in 64 ... 4608", cfg->block_frames);
    if (cfg->sample_rate < 8000 || cfg->sample_rate > 48000) return fl_fail(nullptr, FMD_ERR_ARG, "sample_rate %d outside 8000 ... 48000", cfg->sample_rate);
    if (fmd_device_count() <= 0) return fl_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return fl_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_flac e = new fmd_flac_s();
    e->C = cfg->n_channels; e->S = S; e->fs = cfg->sample_rate; e->max_in = cfg->max_input_frames;
    static const int kRates[11] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000};
    e->sr_code = 13;                                                         // 16 bits of Hz behind the header where the table has no code
    for (int c = 4; c <= 10; c++)
        if (kRates[c] == e->fs) e->sr_code = c;
    e->img_words = (fmd::flac_frame_bound(S) + 3) / 4 + 2;
    const size_t C = (size_t)e->C, n_tab = 256 + (size_t)fmd::flac_frame_bound(S) + kPowSlack;
    std::vector<uint16_t> tab(n_tab);
    fmd::flac_crc16_tables((int)n_tab - 256, tab.data());
    bool ok = e->order.init(dev);
    ok = ok && hipMalloc(&e->d_status, sizeof(fmd_flac_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&e->d_open, sizeof(uint32_t) * (size_t)S * C) == hipSuccess;
    ok = ok && hipMemset(e->d_open, 0, sizeof(uint32_t) * (size_t)S * C) == hipSuccess;
    ok = ok && hipMalloc(&e->d_crc, sizeof(uint16_t) * n_tab) == hipSuccess;
    ok = ok && hipMemcpy(e->d_crc, tab.data(), sizeof(uint16_t) * n_tab, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok || fmd_flac_reset(e, -1) != FMD_OK) {
        fmd_flac_destroy(e);
        return fl_fail(nullptr, FMD_ERR_DEVICE, "device allocation failed");
    }
    *out = e;
    return FMD_OK;
}

int fmd_flac_destroy(fmd_flac e) {
    if (!e) return FMD_ERR_ARG;
    (void)e->order.quiesce();
    for (void* p : {(void*)e->d_status, (void*)e->d_open, (void*)e->d_crc})
        if (p) (void)hipFree(p);
    delete e;
    return FMD_OK;
}

int fmd_flac_reset(fmd_flac e, int channel) {
    if (!e) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, e->C, &c0, &cn)) return fl_fail(e, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, e->C);
    if (!e->order.quiesce()) return fl_fail(e, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_flac_reset, dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, nullptr, c0, cn, e->d_status);
    if (const char* m = fmd::control_end("k_flac_reset launch failed")) return fl_fail(e, FMD_ERR_DEVICE, "%s", m);
    return FMD_OK;
}

int fmd_flac_process_f32_dev(fmd_flac e, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_out, long long out_stride,
                             int* d_nbytes, int* d_nframes, void* stream) {
    if (!e) return FMD_ERR_ARG;
    if (fmd::flac_check_call(e->S, e->max_in, d_in, in_stride, n, d_out, out_stride, &e->err) != FMD_OK) return FMD_ERR_ARG;
    if (n == 0 && !d_nbytes && !d_nframes) return FMD_OK;                    // nothing of any station changes and there is no count to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every station's state carries over from call to call: a caller that switches streams is ordered behind the previous call
    if (const char* m = e->order.begin(s)) return fl_fail(e, FMD_ERR_DEVICE, "%s", m);
    hipLaunchKernelGGL(k_flac, dim3((unsigned)e->C), dim3(kT), e->lds(), s, reinterpret_cast<const fl_f2*>(d_in), in_stride, (int)n, d_active, e->S, e->fs, e->sr_code,
                       e->img_words, e->d_status, e->d_open, e->d_crc, d_out, out_stride, d_nbytes, d_nframes);
    if (hipGetLastError() != hipSuccess) return fl_fail(e, FMD_ERR_DEVICE, "k_flac launch failed");
    if (const char* m = e->order.end(s)) return fl_fail(e, FMD_ERR_DEVICE, "%s", m);
    return FMD_OK;
}

int fmd_flac_flush(fmd_flac e, int channel, uint8_t* d_out, long long out_stride, int* d_nbytes, int* d_nframes, void* stream) {
    if (!e) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, e->C, &c0, &cn)) return fl_fail(e, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, e->C);
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 4 != 0) return fl_fail(e, FMD_ERR_ARG, "null output, or output not aligned to 4 bytes");
    const long long need = fmd::flac_max_bytes(e->S, 1);
    if (out_stride % 4 != 0 || out_stride < need) return fl_fail(e, FMD_ERR_ARG, "out_stride %lld is no multiple of 4 or below a frame's %lld bytes", out_stride, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const char* m = e->order.begin(s)) return fl_fail(e, FMD_ERR_DEVICE, "%s", m);
    hipLaunchKernelGGL(k_flac_flush, dim3((unsigned)cn), dim3(kT), e->lds(), s, c0, e->S, e->fs, e->sr_code, e->img_words, e->d_status, e->d_open, e->d_crc, d_out,
                       out_stride, d_nbytes, d_nframes);
    if (hipGetLastError() != hipSuccess) return fl_fail(e, FMD_ERR_DEVICE, "k_flac_flush launch failed");
    if (const char* m = e->order.end(s)) return fl_fail(e, FMD_ERR_DEVICE, "%s", m);
    return FMD_OK;
}

int fmd_flac_get_status(fmd_flac e, fmd_flac_status* out) {
    if (!e || !out) return fl_fail(e, FMD_ERR_ARG, "null encoder or output");
    if (!e->order.quiesce()) return fl_fail(e, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, e->d_status, sizeof(fmd_flac_status) * (size_t)e->C, hipMemcpyDeviceToHost) != hipSuccess) return fl_fail(e, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_flac_status_dev(fmd_flac e, const fmd_flac_status** d_status) {
    if (!e || !d_status) return fl_fail(e, FMD_ERR_ARG, "null encoder or output");
    *d_status = e->d_status;
    return FMD_OK;
}

const char* fmd_flac_last_error(fmd_flac e) { return e ? e->err.c_str() : fmd::flac_global_error().c_str(); }

int fmd_debug_flac_set_frame_number(fmd_flac e, int channel, unsigned value) {
    if (!e) return FMD_ERR_ARG;
    if (channel < 0 || channel >= e->C || value > 0x7fffffffu) return fl_fail(e, FMD_ERR_ARG, "channel %d outside [0, %d) or a number of 2^31 and above", channel, e->C);
    if (!e->order.quiesce()) return fl_fail(e, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(reinterpret_cast<uint8_t*>(e->d_status + channel) + offsetof(fmd_flac_status, frame_number), &value, sizeof(value), hipMemcpyHostToDevice) != hipSuccess)
        return fl_fail(e, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

}  // extern "C"
