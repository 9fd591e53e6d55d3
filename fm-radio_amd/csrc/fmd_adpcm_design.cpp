// All integer: the tables, the block geometry, the checks, the decoder and the WAV header are the pure functions that
// tests/cpp/adpcm_ref.c restates.
#include "fmd_adpcm_design.h"

#include <cstdio>
#include <cstring>

namespace fmd {

const int kAdpcmStep[kAdpcmSteps] = {FMD_ADPCM_STEP_TABLE};
const int kAdpcmIndexAdjust[8] = {-1, -1, -1, -1, 2, 4, 6, 8};

std::string& adpcm_global_error() {
    thread_local std::string e;
    return e;
}

int adpcm_block_frames(int S) {
    if (S == 0) return kAdpcmDefaultBlock;
    return S < 9 || S > kAdpcmMaxBlock || S % 8 != 1 ? 0 : S;
}

int adpcm_check_call(int S, long long max_in, const void* d_in, long long in_stride, long long n, const void* d_out, long long out_stride, std::string* err) {
    char buf[256];
    auto no = [&](const char* fmt, long long a, long long b) { snprintf(buf, sizeof(buf), fmt, a, b); *err = buf; return FMD_ERR_ARG; };
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8 != 0) return no("null input, or input not aligned to 8 bytes", 0, 0);
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 4 != 0) return no("null output, or output not aligned to 4 bytes", 0, 0);
    if (n < 0 || n > in_stride) return no("n %lld outside [0, in_stride %lld]", n, in_stride);
    if (n > max_in) return no("n %lld above max_input_frames %lld", n, max_in);
    const long long need = ((long long)(S - 1) + n) / S * adpcm_block_align(S);
    if (out_stride % 4 != 0 || out_stride < need) return no("out_stride %lld is no multiple of 4 or below the %lld bytes this call may write", out_stride, need);
    return FMD_OK;
}

}  // namespace fmd

static int ad_fail(int code, const char* msg) {
    fmd::adpcm_global_error() = msg;
    return code;
}

static void ad_put(uint8_t* p, unsigned long long v, int bytes) {
    for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * i));
}

extern "C" {

int fmd_adpcm_block_align(int block_frames) {
    const int S = fmd::adpcm_block_frames(block_frames);
    if (S == 0) return ad_fail(FMD_ERR_ARG, "block_frames is neither 0 nor 1 (mod 8) in 9 ... 8185");
    return fmd::adpcm_block_align(S);
}

long long fmd_adpcm_max_blocks(int block_frames, long long n) {
    const int S = fmd::adpcm_block_frames(block_frames);
    if (S == 0) return ad_fail(FMD_ERR_ARG, "block_frames is neither 0 nor 1 (mod 8) in 9 ... 8185");
    if (n < 0 || n > (1LL << 62)) return ad_fail(FMD_ERR_ARG, "n outside [0, 2^62]");
    return ((long long)(S - 1) + n) / S;
}

int fmd_adpcm_decode_blocks(const uint8_t* blocks, int block_frames, long long n_blocks, int16_t* pcm_out) {
    const int S = fmd::adpcm_block_frames(block_frames);
    if (S == 0) return ad_fail(FMD_ERR_ARG, "block_frames is neither 0 nor 1 (mod 8) in 9 ... 8185");
    if (n_blocks < 0 || (n_blocks > 0 && (!blocks || !pcm_out))) return ad_fail(FMD_ERR_ARG, "n_blocks is negative, or null blocks or output");
    const int align = fmd::adpcm_block_align(S);
    for (long long b = 0; b < n_blocks; b++)                                 // nothing is written for a stream with a header no encoder writes
        if (blocks[b * align + 2] >= fmd::kAdpcmSteps || blocks[b * align + 6] >= fmd::kAdpcmSteps) return ad_fail(FMD_ERR_ARG, "a block header's step index is above 88");
    for (long long b = 0; b < n_blocks; b++) {
        const uint8_t* blk = blocks + b * align;
        int16_t* pcm = pcm_out + b * S * 2;
        for (int rail = 0; rail < 2; rail++) {
            const uint8_t* h = blk + 4 * rail;
            int pred = (int16_t)(uint16_t)(h[0] | (h[1] << 8)), index = h[2];
            pcm[rail] = (int16_t)pred;
            for (int i = 1; i < S; i++) {
                const int k = i - 1;                                         // the code's place: group k / 8, nibble k % 8, the earlier frame low
                const int code = (blk[8 + 8 * (k >> 3) + 4 * rail + ((k & 7) >> 1)] >> (4 * (k & 1))) & 15;
                const int step = fmd::kAdpcmStep[index];
                int vpdiff = step >> 3;
                if (code & 4) vpdiff += step;
                if (code & 2) vpdiff += step >> 1;
                if (code & 1) vpdiff += step >> 2;
                pred = code & 8 ? pred - vpdiff : pred + vpdiff;
                pred = pred > 32767 ? 32767 : pred < -32768 ? -32768 : pred;
                index += fmd::kAdpcmIndexAdjust[code & 7];
                index = index < 0 ? 0 : index > 88 ? 88 : index;
                pcm[2 * i + rail] = (int16_t)pred;
            }
        }
    }
    return FMD_OK;
}

int fmd_adpcm_wav_header(int fs, int block_frames, long long n_blocks, long long n_frames, uint8_t* out, int* len) {
    const int S = fmd::adpcm_block_frames(block_frames);
    if (S == 0) return ad_fail(FMD_ERR_ARG, "block_frames is neither 0 nor 1 (mod 8) in 9 ... 8185");
    if (!out || !len) return ad_fail(FMD_ERR_ARG, "null output");
    if (fs < 1 || fs > 1000000) return ad_fail(FMD_ERR_ARG, "fs outside 1 ... 1000000");
    if (n_blocks < 0 || n_frames < 0 || n_frames > n_blocks * S) return ad_fail(FMD_ERR_ARG, "n_blocks is negative or n_frames outside [0, n_blocks * block_frames]");
    const long long align = fmd::adpcm_block_align(S), data = n_blocks * align;
    if (data > 0xffffffffLL - (fmd::kAdpcmWavHeader - 8)) return ad_fail(FMD_ERR_SIZE, "the blocks do not fit a RIFF file's 32-bit sizes");
    uint8_t* p = out;
    memcpy(p, "RIFF", 4); ad_put(p + 4, (unsigned long long)(fmd::kAdpcmWavHeader - 8 + data), 4); memcpy(p + 8, "WAVE", 4);
    p += 12;
    memcpy(p, "fmt ", 4); ad_put(p + 4, 20, 4);
    ad_put(p + 8, 0x0011, 2);                                                // WAVE_FORMAT_DVI_ADPCM (IMA)
    ad_put(p + 10, 2, 2);                                                    // channels
    ad_put(p + 12, (unsigned long long)fs, 4);
    ad_put(p + 16, (unsigned long long)((long long)fs * align / S), 4);      // nAvgBytesPerSec
    ad_put(p + 20, (unsigned long long)align, 2);                            // nBlockAlign
    ad_put(p + 22, 4, 2);                                                    // wBitsPerSample
    ad_put(p + 24, 2, 2);                                                    // cbSize
    ad_put(p + 26, (unsigned long long)S, 2);                                // wSamplesPerBlock
    p += 28;
    memcpy(p, "fact", 4); ad_put(p + 4, 4, 4); ad_put(p + 8, (unsigned long long)n_frames, 4);
    p += 12;
    memcpy(p, "data", 4); ad_put(p + 4, (unsigned long long)data, 4);
    *len = fmd::kAdpcmWavHeader;
    return FMD_OK;
}

}  // extern "C"
