// The ADPCM encoder's host-only unit (fm-radio_amd/csrc/fmd_adpcm_design.cpp) as a stand-alone program, for a sanitizer build:
//   adpcm_design_main <dir> <S> ...
// Per S given: "<S> <block_align> <max_blocks(S, 0)> <max_blocks(S, 1)> <max_blocks(S, S)> <max_blocks(S, 2048)>", and 5 blocks of
// generated codes with valid headers decoded into a buffer of exactly their size: <dir>/blocks_<S>.u8 and <dir>/pcm_<S>.i16.  Then a
// line of status codes for block sizes that are not valid, one WAV header per S as hex, the header's and the decoder's error codes,
// the process call's checks with each bound from both sides, and "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "fmd_adpcm_design.h"
#include "fmdemod.h"

static void hex(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) std::printf("%02x", b[i]);
    std::printf("\n");
}

static bool dump(const std::string& path, const void* p, size_t n) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, n, f) == n;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    const std::string dir = argv[1];
    uint32_t rng = 12345u;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    for (int a = 2; a < argc; a++) {
        const int S = std::atoi(argv[a]);
        const int align = fmd_adpcm_block_align(S);
        if (align <= 0 || align != fmd::adpcm_block_align(fmd::adpcm_block_frames(S))) return 2;
        std::printf("%d %d %lld %lld %lld %lld\n", S, align, fmd_adpcm_max_blocks(S, 0), fmd_adpcm_max_blocks(S, 1), fmd_adpcm_max_blocks(S, fmd::adpcm_block_frames(S)),
                    fmd_adpcm_max_blocks(S, 2048));
        const int Sv = fmd::adpcm_block_frames(S), nb = 5;
        // heap buffers of exactly the bytes read and written: a sanitizer sees an index one past either
        std::unique_ptr<uint8_t[]> blocks(new uint8_t[(size_t)nb * align]);
        std::unique_ptr<int16_t[]> pcm(new int16_t[(size_t)nb * Sv * 2]);
        for (int i = 0; i < nb * align; i++) blocks[i] = (uint8_t)next();
        for (int b = 0; b < nb; b++) {
            // headers an encoder could have written: index 0, 88 and in between; samples at the ends of the range in the first blocks
            blocks[b * align + 2] = (uint8_t)(b == 0 ? 0 : b == 1 ? 88 : next() % 89);
            blocks[b * align + 6] = (uint8_t)(b == 0 ? 88 : b == 1 ? 0 : next() % 89);
            blocks[b * align + 3] = blocks[b * align + 7] = 0;
            if (b == 0) { blocks[0] = 0xff; blocks[1] = 0x7f; blocks[4] = 0x00; blocks[5] = 0x80; }
        }
        if (fmd_adpcm_decode_blocks(blocks.get(), S, nb, pcm.get()) != FMD_OK) return 3;
        if (!dump(dir + "/blocks_" + std::to_string(Sv) + ".u8", blocks.get(), (size_t)nb * align) ||
            !dump(dir + "/pcm_" + std::to_string(Sv) + ".i16", pcm.get(), (size_t)nb * Sv * 2 * sizeof(int16_t)))
            return 4;
        // a header index above 88: refused, nothing written
        std::unique_ptr<int16_t[]> untouched(new int16_t[(size_t)nb * Sv * 2]);
        std::memset(untouched.get(), 0x55, (size_t)nb * Sv * 2 * sizeof(int16_t));
        blocks[(nb - 1) * align + 6] = 89;
        if (fmd_adpcm_decode_blocks(blocks.get(), S, nb, untouched.get()) != FMD_ERR_ARG) return 5;
        for (int i = 0; i < nb * Sv * 2; i++)
            if (untouched[i] != 0x5555) return 6;
        if (fmd_adpcm_decode_blocks(nullptr, S, 0, nullptr) != FMD_OK || fmd_adpcm_decode_blocks(nullptr, S, 1, pcm.get()) != FMD_ERR_ARG ||
            fmd_adpcm_decode_blocks(blocks.get(), S, -1, pcm.get()) != FMD_ERR_ARG)
            return 7;
    }
    for (int S : {1, 8, 10, 16, 1016, 1018, 1025, 8177, 8186, 8193, -7}) std::printf("%d %lld %d ", fmd_adpcm_block_align(S), fmd_adpcm_max_blocks(S, 5), fmd::adpcm_block_frames(S));
    std::printf("%lld %lld\n", fmd_adpcm_max_blocks(9, -1), fmd_adpcm_max_blocks(9, 1LL << 62));
    for (int a = 2; a < argc; a++) {
        const int S = std::atoi(argv[a]), Sv = fmd::adpcm_block_frames(S);
        std::unique_ptr<uint8_t[]> h(new uint8_t[FMD_ADPCM_WAV_HEADER_BYTES]);
        int len = 0;
        if (fmd_adpcm_wav_header(32000 + a, S, 7, 7LL * Sv - 3, h.get(), &len) != FMD_OK || len != FMD_ADPCM_WAV_HEADER_BYTES) return 8;
        hex(h.get(), (size_t)len);
    }
    {
        uint8_t h[FMD_ADPCM_WAV_HEADER_BYTES];
        int len = -1;
        const long long big = (0xffffffffLL - 52) / 1024;                    // the most blocks of 1024 bytes a RIFF size holds
        std::printf("%d %d %d %d %d %d %d %d %d %d %d\n", fmd_adpcm_wav_header(0, 0, 1, 1, h, &len), fmd_adpcm_wav_header(1, 0, 1, 1, h, &len),
                    fmd_adpcm_wav_header(1000000, 0, 1, 1, h, &len), fmd_adpcm_wav_header(1000001, 0, 1, 1, h, &len), fmd_adpcm_wav_header(32000, 0, -1, 0, h, &len),
                    fmd_adpcm_wav_header(32000, 0, 1, 1017, h, &len), fmd_adpcm_wav_header(32000, 0, 1, 1018, h, &len), fmd_adpcm_wav_header(32000, 0, 1, -1, h, &len),
                    fmd_adpcm_wav_header(32000, 0, big, 0, h, &len), fmd_adpcm_wav_header(32000, 0, big + 1, 0, h, &len), fmd_adpcm_wav_header(32000, 12, 1, 1, h, &len));
        if (fmd_adpcm_wav_header(32000, 0, 1, 1, nullptr, &len) != FMD_ERR_ARG || fmd_adpcm_wav_header(32000, 0, 1, 1, h, nullptr) != FMD_ERR_ARG) return 9;
    }
    {
        // the process call's checks for S = 17 (24 bytes a block) and max_input_frames = 100: a call of 40 frames may complete
        // (16 + 40) / 17 = 3 blocks, 72 bytes
        alignas(16) static unsigned char mem[64];
        std::string err;
        auto chk = [&](const void* in, long long in_stride, long long n, const void* out, long long out_stride) {
            return fmd::adpcm_check_call(17, 100, in, in_stride, n, out, out_stride, &err);
        };
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", chk(mem, 40, 40, mem, 72), chk(mem, 40, 40, mem, 68), chk(mem, 40, 40, mem, 74), chk(mem, 40, 40, mem, 76),
                    chk(mem, 40, 0, mem, 0), chk(mem, 40, -1, mem, 72), chk(mem, 40, 41, mem, 96), chk(mem, 41, 41, mem, 72), chk(mem, 200, 100, mem, 144),
                    chk(mem, 200, 101, mem, 168), chk(mem + 8, 40, 40, mem, 72), chk(mem + 4, 40, 40, mem, 72), chk(mem, 40, 40, mem + 4, 72), chk(mem, 40, 40, mem + 2, 72),
                    chk(nullptr, 40, 40, mem, 72), chk(mem, 40, 40, nullptr, 72));
        if (err.empty()) return 10;
    }
    std::printf("ok\n");
    return 0;
}
