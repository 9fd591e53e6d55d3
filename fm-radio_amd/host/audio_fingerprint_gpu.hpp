// Header-only C++ host adaptor over the C ABI's audio fingerprinter (include/fmdemod.h "Audio fingerprinter"): RAII around the handle, the
// output words [C][max_prints] uint32 for a given max_input_frames and the [C] counts on the device, exceptions instead of status codes,
// and per-station views.  NOT in the reference (williamyang98/FM-Radio plays one station to a listener): it reads the station audio
// [C][in_stride][2] f32 that the mixer and the monitors read, and what it writes is what a host ships to a fingerprint database or
// compares across stations:
//
//   fmd_host::AudioFingerprint_GPU fp(n_channels, 32000, frames_per_block);   // the default geometry: 368 / 32 / 33 bands
//   fp.Process(d_audio, in_stride, n, nullptr, stream);                        // asynchronous on the stream given
//   fp.Update();                                                               // waits, copies counts, records and words to the host
//   fp.Prints(c); fp.Word(c, i); fp.WordTime(c, i);
//   fmd_host::AudioFingerprint_GPU::BitErrorRate(a, b, n);                      // two runs of n words: compare with the paper's 0.35
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class AudioFingerprint_GPU {
    fmd_fprint h = nullptr;
    fmd_fprint_config cfg{};
    long long max_prints = 0;
    uint32_t* d_out = nullptr;               // [C][max_prints]
    int* d_counts = nullptr;                 // [C]
    std::vector<fmd_fprint_status> status;
    std::vector<int> counts;
    std::vector<uint32_t> words;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_fprint_last_error(h)); }
    void init() {
        if (fmd_fprint_create(&cfg, &h) != FMD_OK) throw std::runtime_error(std::string("fmd_fprint_create: ") + fmd_fprint_last_error(nullptr));
        max_prints = fmd_fprint_max_prints(cfg.hop, cfg.max_input_frames);
        const size_t C = (size_t)cfg.n_channels;
        status.resize(C); counts.assign(C, 0); words.assign(C * (size_t)max_prints, 0u);
        // (create has made `device` current where one was given); before the first Process every count is 0
        if (hipMalloc(reinterpret_cast<void**>(&d_out), sizeof(uint32_t) * words.size()) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&d_counts), sizeof(int) * C) != hipSuccess ||
            hipMemset(d_out, 0, sizeof(uint32_t) * words.size()) != hipSuccess || hipMemset(d_counts, 0, sizeof(int) * C) != hipSuccess) {
            release();
            throw std::runtime_error("AudioFingerprint_GPU: the output's allocation failed");
        }
    }
    void release() {
        if (h) fmd_fprint_destroy(h);
        if (d_out) (void)hipFree(d_out);
        if (d_counts) (void)hipFree(d_counts);
        h = nullptr; d_out = nullptr; d_counts = nullptr;
    }
public:
    // the default geometry at the audio's own rate
    AudioFingerprint_GPU(int n_channels, int fs, long long max_input_frames, int device = -1) {
        if (fmd_fprint_default_config(fs, &cfg) != FMD_OK) throw std::runtime_error(std::string("fmd_fprint_default_config: ") + fmd_fprint_last_error(nullptr));
        cfg.n_channels = n_channels; cfg.max_input_frames = max_input_frames; cfg.device = device;
        init();
    }
    explicit AudioFingerprint_GPU(const fmd_fprint_config& _cfg) : cfg(_cfg) { init(); }
    ~AudioFingerprint_GPU() { release(); }
    AudioFingerprint_GPU(const AudioFingerprint_GPU&) = delete;
    AudioFingerprint_GPU& operator=(const AudioFingerprint_GPU&) = delete;

    int GetTotalChannels() const { return cfg.n_channels; }
    const fmd_fprint_config& Config() const { return cfg; }
    long long MaxPrints() const { return max_prints; }       // words a station's view holds: also the stride from one station to the next
    int BitsPerWord() const { return cfg.n_bands - 1; }
    long long StateBytes() const { return fmd_fprint_state_bytes(&cfg, cfg.n_channels); }

    // takes n <= max_input_frames frames of every station whose d_active byte is not 0 (NULL: all); asynchronous on `stream`
    void Process(const float* d_in, long long in_stride, long long n, const unsigned char* d_active = nullptr, void* stream = nullptr) {
        check(fmd_fprint_process_f32_dev(h, d_in, in_stride, n, d_active, d_out, max_prints, d_counts, nullptr, 0, stream), "fmd_fprint_process_f32_dev");
    }
    void Reset(int channel = -1) { check(fmd_fprint_reset(h, channel), "fmd_fprint_reset"); }

    // the device's views, written behind every Process on its stream: station c's words [MaxPrints()], of which the first
    // CountsDev()[c] are the last call's
    const uint32_t* WordsDev(int c) const { return d_out + (size_t)c * (size_t)max_prints; }
    const int* CountsDev() const { return d_counts; }
    const fmd_fprint_status* StatusDev() const {
        const fmd_fprint_status* p = nullptr;
        check(fmd_fprint_status_dev(h, &p), "fmd_fprint_status_dev");
        return p;
    }

    // waits for the object's work and copies every station's record, count and words to the host
    void Update() {
        check(fmd_fprint_get_status(h, status.data()), "fmd_fprint_get_status");
        if (hipMemcpy(counts.data(), d_counts, sizeof(int) * counts.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(words.data(), d_out, sizeof(uint32_t) * words.size(), hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error("AudioFingerprint_GPU: the output's copy failed");
    }
    // as of the last Update()
    const fmd_fprint_status& Status(int c) const { return status.at((size_t)c); }
    int Prints(int c) const { return counts.at((size_t)c); }
    uint32_t Word(int c, int i) const {
        if (i < 0 || i >= Prints(c)) throw std::out_of_range("AudioFingerprint_GPU::Word");
        return words[(size_t)c * (size_t)max_prints + (size_t)i];
    }
    // the start of word i of the last call in seconds since the station's reset: sample (index + 1) hop
    double WordTime(int c, int i) const {
        const unsigned long long first = Status(c).prints - (unsigned long long)Prints(c);
        return (double)(first + (unsigned long long)i + 1ull) * (double)cfg.hop / (double)cfg.fs;
    }
    // differing bits among the top `bits` of each word of two runs of n words, over their number
    static double BitErrorRate(const uint32_t* a, const uint32_t* b, size_t n, int bits = 32) {
        if (n == 0 || bits < 1 || bits > 32) throw std::invalid_argument("AudioFingerprint_GPU::BitErrorRate");
        unsigned long long errs = 0;
        for (size_t i = 0; i < n; i++) errs += (unsigned long long)__builtin_popcount((a[i] ^ b[i]) >> (32 - bits));
        return (double)errs / ((double)n * (double)bits);
    }
};

}  // namespace fmd_host
