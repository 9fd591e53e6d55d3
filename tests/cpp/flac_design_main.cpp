// The FLAC encoder's host-only unit (fm-radio_amd/csrc/fmd_flac_design.cpp) as a stand-alone program, for a sanitizer build:
//   flac_design_main <dir> <fs> <S> <stream file> [<fs> <S> <stream file> ...]
// Per stream (one station's FLAC frames as the restatement wrote them): the frames decoded into a buffer of exactly their size,
// <dir>/pcm_<index>.i16; a line "<frames> <code with a buffer one frame short> <prefix lengths that decode, ...>" over every prefix of
// the stream, each in a heap buffer of exactly its length; a line "<single-bit corruptions tried> <of those refused>".  Then the bounds
// for valid and invalid block sizes, stream headers as hex, the header's and the decoder's error codes, the process call's checks with
// each bound from both sides, the two CRC check values, and "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fmd_flac_design.h"
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

static bool slurp(const char* path, std::vector<uint8_t>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[4096];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + k);
    return std::fclose(f) == 0;
}

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 2) % 3 != 0) return 1;
    const std::string dir = argv[1];
    for (int a = 2, index = 0; a + 2 < argc; a += 3, index++) {
        const int fs = std::atoi(argv[a]), S = std::atoi(argv[a + 1]);
        std::vector<uint8_t> file;
        if (!slurp(argv[a + 2], file)) return 2;
        const long long len = (long long)file.size();
        // heap buffers of exactly the bytes read and written: a sanitizer sees an index one past either
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[(size_t)len]);
        std::memcpy(bytes.get(), file.data(), (size_t)len);
        long long frames = -1, again = -1;
        if (fmd_flac_decode(bytes.get(), len, fs, S, nullptr, 0, &frames) != FMD_OK || frames <= 0) return 3;
        std::unique_ptr<int16_t[]> pcm(new int16_t[(size_t)frames * 2]);
        if (fmd_flac_decode(bytes.get(), len, fs, S, pcm.get(), frames, &again) != FMD_OK || again != frames) return 4;
        if (!dump(dir + "/pcm_" + std::to_string(index) + ".i16", pcm.get(), (size_t)frames * 2 * sizeof(int16_t))) return 5;
        std::unique_ptr<int16_t[]> shorter(new int16_t[(size_t)(frames - 1) * 2 + 1]);
        std::printf("%lld %d", frames, fmd_flac_decode(bytes.get(), len, fs, S, shorter.get(), frames - 1, &again));
        for (long long cut = 0; cut < len; cut++) {
            std::unique_ptr<uint8_t[]> part(new uint8_t[(size_t)cut + 1]);   // (one spare byte that no call is told of: new[0] may not be read at all)
            std::memcpy(part.get(), bytes.get(), (size_t)cut);
            const int rc = fmd_flac_decode(cut ? part.get() : nullptr, cut, fs, S, pcm.get(), frames, &again);
            if (rc == FMD_OK) std::printf(" %lld", cut);
            else if (rc != FMD_ERR_ARG) return 6;
        }
        std::printf("\n");
        int tried = 0, refused = 0;
        for (long long bit = 0; bit < 8 * len; bit += (bit < 8 * 64 ? 1 : 37)) {
            bytes[(size_t)(bit >> 3)] ^= (uint8_t)(0x80u >> (bit & 7));
            tried++;
            refused += fmd_flac_decode(bytes.get(), len, fs, S, pcm.get(), frames, &again) == FMD_ERR_ARG;
            bytes[(size_t)(bit >> 3)] ^= (uint8_t)(0x80u >> (bit & 7));
        }
        std::printf("%d %d\n", tried, refused);
        if (fmd_flac_decode(bytes.get(), len, fs == 32000 ? 44100 : 32000, S, pcm.get(), frames, &again) != FMD_ERR_ARG) return 7;      // another rate
        if (fmd_flac_decode(bytes.get(), -1, fs, S, pcm.get(), frames, &again) != FMD_ERR_ARG || fmd_flac_decode(nullptr, 1, fs, S, pcm.get(), frames, &again) != FMD_ERR_ARG ||
            fmd_flac_decode(bytes.get(), len, fs, S, nullptr, 1, &again) != FMD_ERR_ARG || fmd_flac_decode(bytes.get(), len, fs, S, pcm.get(), frames, nullptr) != FMD_ERR_ARG ||
            fmd_flac_decode(bytes.get(), len, 7999, S, pcm.get(), frames, &again) != FMD_ERR_ARG || fmd_flac_decode(bytes.get(), len, fs, 65, pcm.get(), frames, &again) != FMD_ERR_ARG)
            return 8;
    }
    for (int S : {0, 64, 128, 576, 4096, 4608, 1, 63, 65, 96, 4544, 4609, 4672, -64})
        std::printf("%d %lld %lld %lld %d ", fmd_flac_frame_bound(S), fmd_flac_max_bytes(S, 0), fmd_flac_max_bytes(S, 1), fmd_flac_max_bytes(S, 2048), fmd::flac_block_frames(S));
    std::printf("%lld %lld %lld\n", fmd_flac_max_bytes(64, -1), fmd_flac_max_bytes(64, 1LL << 40), fmd_flac_max_bytes(64, (1LL << 40) + 1));
    for (int S : {0, 64, 4608}) {
        std::unique_ptr<uint8_t[]> h(new uint8_t[FMD_FLAC_STREAM_HEADER_BYTES]);
        int len = 0;
        if (fmd_flac_stream_header(32000 + S, S, (1LL << 36) - 1 - S, 14 + S, 12345 + S, h.get(), &len) != FMD_OK || len != FMD_FLAC_STREAM_HEADER_BYTES) return 9;
        hex(h.get(), (size_t)len);
    }
    {
        uint8_t h[FMD_FLAC_STREAM_HEADER_BYTES];
        int len = -1;
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", fmd_flac_stream_header(7999, 0, 0, 0, 0, h, &len), fmd_flac_stream_header(8000, 0, 0, 0, 0, h, &len),
                    fmd_flac_stream_header(48000, 0, 0, 0, 0, h, &len), fmd_flac_stream_header(48001, 0, 0, 0, 0, h, &len), fmd_flac_stream_header(32000, 0, -1, 0, 0, h, &len),
                    fmd_flac_stream_header(32000, 0, (1LL << 36) - 1, 0, 0, h, &len), fmd_flac_stream_header(32000, 0, 1LL << 36, 0, 0, h, &len),
                    fmd_flac_stream_header(32000, 0, 0, -1, 0, h, &len), fmd_flac_stream_header(32000, 0, 0, 5, 4, h, &len), fmd_flac_stream_header(32000, 0, 0, 5, 5, h, &len),
                    fmd_flac_stream_header(32000, 0, 0, 0, (1 << 24) - 1, h, &len), fmd_flac_stream_header(32000, 0, 0, 0, 1 << 24, h, &len),
                    fmd_flac_stream_header(32000, 100, 0, 0, 0, h, &len));
        if (fmd_flac_stream_header(32000, 0, 0, 0, 0, nullptr, &len) != FMD_ERR_ARG || fmd_flac_stream_header(32000, 0, 0, 0, 0, h, nullptr) != FMD_ERR_ARG) return 10;
    }
    {
        // the process call's checks for S = 64 (a frame's bound 276 bytes) and max_input_frames = 100: a call of 70 frames may complete
        // (63 + 70) / 64 = 2 frames, 552 bytes
        alignas(16) static unsigned char mem[64];
        std::string err;
        auto chk = [&](const void* in, long long in_stride, long long n, const void* out, long long out_stride) {
            return fmd::flac_check_call(64, 100, in, in_stride, n, out, out_stride, &err);
        };
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", chk(mem, 70, 70, mem, 552), chk(mem, 70, 70, mem, 548), chk(mem, 70, 70, mem, 554), chk(mem, 70, 70, mem, 556),
                    chk(mem, 70, 0, mem, 0), chk(mem, 70, -1, mem, 552), chk(mem, 70, 71, mem, 1104), chk(mem, 71, 71, mem, 552), chk(mem, 200, 100, mem, 552),
                    chk(mem, 200, 101, mem, 552), chk(mem + 8, 70, 70, mem, 552), chk(mem + 4, 70, 70, mem, 552), chk(mem, 70, 70, mem + 4, 552), chk(mem, 70, 70, mem + 2, 552),
                    chk(nullptr, 70, 70, mem, 552), chk(mem, 70, 70, nullptr, 552));
        if (err.empty()) return 11;
    }
    std::printf("%02x %04x\n", fmd::flac_crc8(reinterpret_cast<const uint8_t*>("123456789"), 9), fmd::flac_crc16(reinterpret_cast<const uint8_t*>("123456789"), 9));
    {
        // the kernels' tables: the byte table is the CRC of each byte, and crc(A | B) = crc(A) * x^(8 |B|) + crc(B) with the table's factor
        std::unique_ptr<uint16_t[]> tab(new uint16_t[256 + 40]);
        fmd::flac_crc16_tables(40, tab.get());
        const uint8_t* msg = reinterpret_cast<const uint8_t*>("123456789 and the rest of it");
        const unsigned ca = fmd::flac_crc16(msg, 9), cb = fmd::flac_crc16(msg + 9, 19), whole = fmd::flac_crc16(msg, 28);
        unsigned r = 0, b = tab[256 + 19];
        for (int i = 15; i >= 0; i--) {
            r = (r << 1) ^ ((r & 0x8000u) ? 0x18005u : 0u);
            if ((b >> i) & 1u) r ^= ca;
        }
        for (unsigned i = 0; i < 256; i++) {
            const uint8_t byte = (uint8_t)i;
            if (tab[i] != fmd::flac_crc16(&byte, 1)) return 12;
        }
        if (((r & 0xffffu) ^ cb) != whole || tab[256] != 1 || tab[257] != 0x0100) return 13;
    }
    std::printf("ok\n");
    return 0;
}
