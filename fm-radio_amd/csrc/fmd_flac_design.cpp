// All integer: the geometry, the checks, the CRC tables, the stream header and the decoder are the pure functions that
// tests/cpp/flac_ref.c and tests/flac_ref.py restate.
#include "fmd_flac_design.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace fmd {

std::string& flac_global_error() {
    thread_local std::string e;
    return e;
}

int flac_block_frames(int S) {
    if (S == 0) return kFlacDefaultBlock;
    return S < 64 || S > kFlacMaxBlock || S % 64 != 0 ? 0 : S;
}

int flac_check_call(int S, long long max_in, const void* d_in, long long in_stride, long long n, const void* d_out, long long out_stride, std::string* err) {
    char buf[256];
    auto no = [&](const char* fmt, long long a, long long b) { snprintf(buf, sizeof(buf), fmt, a, b); *err = buf; return FMD_ERR_ARG; };
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return no("null input, or input not aligned to 8 bytes", 0, 0);
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 4 != 0) return no("null output, or output not aligned to 4 bytes", 0, 0);
    if (n < 0 || n > in_stride) return no("n %lld outside [0, in_stride %lld]", n, in_stride);
    if (n > max_in) return no("n %lld above max_input_frames %lld", n, max_in);
    const long long need = flac_max_bytes(S, n);
    if (out_stride % 4 != 0 || out_stride < need) return no("out_stride %lld is no multiple of 4 or below the %lld bytes this call may write", out_stride, need);
    return FMD_OK;
}

static unsigned crc16_byte(unsigned c) {
    c <<= 8;
    for (int b = 0; b < 8; b++) c = (c & 0x8000u) ? ((c << 1) ^ kFlacCrc16Poly) & 0xffffu : (c << 1) & 0xffffu;
    return c;
}

void flac_crc16_tables(int n_pow, uint16_t* out) {
    for (unsigned i = 0; i < 256; i++) out[i] = (uint16_t)crc16_byte(i);
    unsigned v = 1;                                                          // x^0
    for (int m = 0; m < n_pow; m++) {
        out[256 + m] = (uint16_t)v;
        v = ((v << 8) & 0xffffu) ^ out[v >> 8];                              // times x^8: eight zero bits through the register
    }
}

unsigned flac_crc8(const uint8_t* p, long long n) {
    unsigned c = 0;
    for (long long i = 0; i < n; i++) {
        c ^= p[i];
        for (int b = 0; b < 8; b++) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xffu : (c << 1) & 0xffu;
    }
    return c;
}

unsigned flac_crc16(const uint8_t* p, long long n) {
    unsigned c = 0;
    for (long long i = 0; i < n; i++) c = ((c << 8) & 0xffffu) ^ crc16_byte((c >> 8) ^ p[i]);
    return c;
}

}  // namespace fmd

static int fl_fail(int code, const char* msg) {
    fmd::flac_global_error() = msg;
    return code;
}

namespace {

// a frame's bits, MSB first; every read is checked against the end
struct BitReader {
    const uint8_t* p;
    long long bits, pos;
    bool ok = true;
    unsigned get(int n) {                                                    // n <= 24
        if (pos + n > bits) { ok = false; pos = bits; return 0; }
        unsigned v = 0;
        for (int i = 0; i < n; i++, pos++) v = (v << 1) | ((p[pos >> 3] >> (7 - (pos & 7))) & 1u);
        return v;
    }
    int sget(int n) {
        const unsigned v = get(n);
        return (v >> (n - 1)) & 1u ? (int)v - (1 << n) : (int)v;
    }
    long long unary() {
        long long q = 0;
        for (;;) {
            if (pos >= bits) { ok = false; return 0; }
            const unsigned b = (p[pos >> 3] >> (7 - (pos & 7))) & 1u;
            pos++;
            if (b) return q;
            q++;
        }
    }
};

const int kBlockSizes[16] = {0, 192, 576, 1152, 2304, 4608, 0, 0, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768};
const int kRates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};

bool table_block(int n) {
    for (int c = 1; c < 16; c++)
        if (kBlockSizes[c] == n) return true;
    return false;
}

// one subframe of n samples of bps bits into x; false for anything outside the encoder's subset or a frame that ends early
bool subframe(BitReader& r, int n, int bps, std::vector<long long>& x) {
    x.clear();
    if (r.get(1) != 0) return false;
    const unsigned kind = r.get(6);
    if (r.get(1) != 0 || !r.ok) return false;                                // wasted bits: not built
    if (kind == 0) {
        const int v = r.sget(bps);
        x.assign((size_t)n, v);
        return r.ok;
    }
    if (kind == 1) {
        for (int i = 0; i < n && r.ok; i++) x.push_back(r.sget(bps));
        return r.ok;
    }
    if (kind < 8 || kind > 12) return false;
    const int o = (int)kind - 8;
    if (o >= n) return false;                                                // (a block of o samples and no residual is CONSTANT or VERBATIM here)
    for (int i = 0; i < o; i++) x.push_back(r.sget(bps));
    if (r.get(2) != 0) return false;                                         // method 00 only
    const int p = (int)r.get(4);
    if (!r.ok || p > 6 || n % (1 << p) != 0 || (p > 0 && (n >> p) <= o)) return false;
    for (int j = 0; j < (1 << p); j++) {
        const int k = (int)r.get(4);
        if (!r.ok || k == 15) return false;                                  // no escape partitions
        const int cnt = (n >> p) - (j == 0 ? o : 0);
        for (int t = 0; t < cnt; t++) {
            const long long q = r.unary();
            const unsigned low = r.get(k);
            if (!r.ok || q > (1LL << 24)) return false;
            const long long u = (q << k) | low, res = (u & 1) ? -((u + 1) >> 1) : (u >> 1);
            const size_t i = x.size();
            long long pred = 0;
            if (o == 1) pred = x[i - 1];
            if (o == 2) pred = 2 * x[i - 1] - x[i - 2];
            if (o == 3) pred = 3 * x[i - 1] - 3 * x[i - 2] + x[i - 3];
            if (o == 4) pred = 4 * x[i - 1] - 6 * x[i - 2] + 4 * x[i - 3] - x[i - 4];
            const long long v = pred + res;
            if (v < -(1LL << (bps - 1)) || v >= (1LL << (bps - 1))) return false;
            x.push_back(v);
        }
    }
    return true;
}

}  // namespace

extern "C" {

int fmd_flac_frame_bound(int block_frames) {
    const int S = fmd::flac_block_frames(block_frames);
    if (S == 0) return fl_fail(FMD_ERR_ARG, "block_frames is neither 0 nor a multiple of 64 in 64 ... 4608");
    return fmd::flac_frame_bound(S);
}

long long fmd_flac_max_bytes(int block_frames, long long n) {
    const int S = fmd::flac_block_frames(block_frames);
    if (S == 0) return fl_fail(FMD_ERR_ARG, "block_frames is neither 0 nor a multiple of 64 in 64 ... 4608");
    if (n < 0 || n > (1LL << 40)) return fl_fail(FMD_ERR_ARG, "n outside [0, 2^40]");
    return fmd::flac_max_bytes(S, n);
}

int fmd_flac_stream_header(int fs, int block_frames, long long total_samples, int min_frame_bytes, int max_frame_bytes, uint8_t* out, int* len) {
    const int S = fmd::flac_block_frames(block_frames);
    if (S == 0) return fl_fail(FMD_ERR_ARG, "block_frames is neither 0 nor a multiple of 64 in 64 ... 4608");
    if (!out || !len) return fl_fail(FMD_ERR_ARG, "null output");
    if (fs < 8000 || fs > 48000) return fl_fail(FMD_ERR_ARG, "fs outside 8000 ... 48000");
    if (total_samples < 0 || total_samples >= (1LL << 36)) return fl_fail(FMD_ERR_ARG, "total_samples outside [0, 2^36)");
    if (min_frame_bytes < 0 || max_frame_bytes < 0 || max_frame_bytes >= (1 << 24) || min_frame_bytes > max_frame_bytes)
        return fl_fail(FMD_ERR_ARG, "frame bytes negative, 2^24 or more, or min above max");
    uint8_t* p = out;
    memcpy(p, "fLaC", 4);
    p[4] = 0x80;                                                             // the last metadata block, type 0 = STREAMINFO
    p[5] = 0; p[6] = 0; p[7] = 34;
    p[8] = (uint8_t)(S >> 8); p[9] = (uint8_t)S;                             // min = max block size
    p[10] = (uint8_t)(S >> 8); p[11] = (uint8_t)S;
    p[12] = (uint8_t)(min_frame_bytes >> 16); p[13] = (uint8_t)(min_frame_bytes >> 8); p[14] = (uint8_t)min_frame_bytes;
    p[15] = (uint8_t)(max_frame_bytes >> 16); p[16] = (uint8_t)(max_frame_bytes >> 8); p[17] = (uint8_t)max_frame_bytes;
    // 20 bits of rate, 3 of channels - 1, 5 of bits - 1, 36 of total samples
    const unsigned long long v = ((unsigned long long)fs << 44) | (1ULL << 41) | (15ULL << 36) | (unsigned long long)total_samples;
    for (int i = 0; i < 8; i++) p[18 + i] = (uint8_t)(v >> (56 - 8 * i));
    memset(p + 26, 0, 16);                                                   // MD5 of the samples: all zero = not computed
    *len = fmd::kFlacStreamHeader;
    return FMD_OK;
}

int fmd_flac_decode(const uint8_t* bytes, long long len, int fs, int block_frames, int16_t* pcm_out, long long cap, long long* n_frames_out) {
    const int S = fmd::flac_block_frames(block_frames);
    if (S == 0) return fl_fail(FMD_ERR_ARG, "block_frames is neither 0 nor a multiple of 64 in 64 ... 4608");
    if (fs < 8000 || fs > 48000) return fl_fail(FMD_ERR_ARG, "fs outside 8000 ... 48000");
    if (len < 0 || (len > 0 && !bytes) || cap < 0 || (cap > 0 && !pcm_out) || !n_frames_out) return fl_fail(FMD_ERR_ARG, "negative length or capacity, or a null pointer");
    long long at = 0, total = 0;
    unsigned number = 0;
    bool short_seen = false;
    std::vector<long long> c0, c1;
    while (at < len) {
        if (short_seen) return fl_fail(FMD_ERR_ARG, "a frame behind a short frame");
        const uint8_t* d = bytes + at;
        const long long left = len - at;
        if (left < 6 || d[0] != 0xff || d[1] != 0xf8) return fl_fail(FMD_ERR_ARG, "no sync code, a reserved bit, or a variable-blocksize frame");
        const int bs_code = d[2] >> 4, sr_code = d[2] & 15, ch_code = d[3] >> 4, ss_code = (d[3] >> 1) & 7;
        if ((d[3] & 1) || ss_code != 4 || !(ch_code == 1 || ch_code == 8 || ch_code == 9 || ch_code == 10) || bs_code == 0 || sr_code == 0 || sr_code > 13 || sr_code == 12)
            return fl_fail(FMD_ERR_ARG, "a reserved bit or code, or a header this encoder does not write");
        const unsigned first = d[4];
        const int extra = first < 0x80 ? 0 : (first >> 5) == 6 ? 1 : (first >> 4) == 14 ? 2 : (first >> 3) == 30 ? 3 : (first >> 2) == 62 ? 4 : (first >> 1) == 126 ? 5 : -1;
        if (extra < 0 || left < 5 + extra + 1) return fl_fail(FMD_ERR_ARG, "the coded frame number");
        unsigned v = extra == 0 ? first : first & (0x3fu >> extra);
        for (int i = 0; i < extra; i++) {
            if ((d[5 + i] >> 6) != 2) return fl_fail(FMD_ERR_ARG, "the coded frame number");
            v = (v << 6) | (d[5 + i] & 0x3fu);
        }
        static const unsigned kLeast[6] = {0, 0x80u, 0x800u, 0x10000u, 0x200000u, 0x4000000u};
        if (v < kLeast[extra] || v != number) return fl_fail(FMD_ERR_ARG, "a frame number out of sequence or coded longer than needed");
        long long p = 5 + extra;
        const long long need = p + (bs_code == 6 ? 1 : bs_code == 7 ? 2 : 0) + (sr_code == 13 ? 2 : 0) + 1;
        if (left < need) return fl_fail(FMD_ERR_ARG, "the stream ends inside a frame header");
        int n = kBlockSizes[bs_code];
        if (bs_code == 6) { n = d[p] + 1; p += 1; }
        if (bs_code == 7) { n = ((d[p] << 8) | d[p + 1]) + 1; p += 2; }
        if ((bs_code == 6 || bs_code == 7) && (table_block(n) || (bs_code == 7 && n <= 256))) return fl_fail(FMD_ERR_ARG, "a block size not coded the encoder's way");
        int rate = sr_code <= 11 ? kRates[sr_code] : 0;
        if (sr_code == 13) {
            rate = (d[p] << 8) | d[p + 1]; p += 2;
            for (int c = 1; c <= 11; c++)
                if (kRates[c] == rate) return fl_fail(FMD_ERR_ARG, "a sample rate not coded the encoder's way");
        }
        if (rate != fs || n > S) return fl_fail(FMD_ERR_ARG, "a frame of another sample rate or above the block size");
        if (fmd::flac_crc8(d, p) != d[p]) return fl_fail(FMD_ERR_ARG, "CRC-8");
        p += 1;
        BitReader r{d, 8 * left, 8 * p};
        if (!subframe(r, n, ch_code == 9 ? 17 : 16, c0) || !subframe(r, n, ch_code == 8 || ch_code == 10 ? 17 : 16, c1))
            return fl_fail(FMD_ERR_ARG, "a subframe outside the encoder's subset, or the stream ends inside it");
        if (r.get((int)((8 - (r.pos & 7)) & 7)) != 0 || !r.ok) return fl_fail(FMD_ERR_ARG, "padding bits set");
        const long long end = r.pos >> 3;
        if (end + 2 > left || fmd::flac_crc16(d, end) != (unsigned)((d[end] << 8) | d[end + 1])) return fl_fail(FMD_ERR_ARG, "CRC-16");
        if (pcm_out && total + n > cap) return fl_fail(FMD_ERR_SIZE, "pcm_out holds fewer frames than the stream");
        for (int i = 0; i < n; i++) {
            long long l = c0[(size_t)i], rr = c1[(size_t)i];
            if (ch_code == 8) rr = l - rr;
            else if (ch_code == 9) l = l + rr;
            else if (ch_code == 10) {
                const long long mid = l * 2 + (rr & 1), side = rr;
                l = (mid + side) >> 1; rr = (mid - side) >> 1;
            }
            if (l < -32768 || l > 32767 || rr < -32768 || rr > 32767) return fl_fail(FMD_ERR_ARG, "a decoded sample outside 16 bits");
            if (pcm_out) { pcm_out[2 * (total + i)] = (int16_t)l; pcm_out[2 * (total + i) + 1] = (int16_t)rr; }
        }
        total += n;
        short_seen = n != S;
        number++;
        at += end + 2;
    }
    *n_frames_out = total;
    return FMD_OK;
}

}  // extern "C"
