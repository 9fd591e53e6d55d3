// Header-only C++ host adaptor over the C ABI's fingerprint matcher (include/fmdemod.h "Fingerprint matcher"): RAII around the handle,
// the events [C][max_events], their counts [C] and the flags and ok bytes [C] on the device, exceptions instead of status codes, and
// per-station views.  NOT in the reference (williamyang98/FM-Radio plays one station to a listener).  It takes what
// AudioFingerprint_GPU writes, on the device, with no host round trip:
//
//   fmd_host::FingerprintMatcher_GPU fm(cfg);                                  // fmd_fpmatch_default_config, then n_channels, max_words ...
//   fm.Load(words, starts, n_tracks);                                           // the catalogue, from host memory
//   fm.Process(fp.WordsDev(0), fp.MaxPrints(), fp.CountsDev(), fp.MaxPrints(), nullptr, stream);   // behind the fingerprinter, same stream
//   fm.OkDev();                                                                 // [C] uint8 for a mixer bus or a recorder's d_active
//   fm.Update(); fm.Status(c).track; fm.Events(c); fm.Event(c, i);
//
// With an index configuration the object searches through the catalogue's index instead of by brute force (fmd_fpmatch_create_ex):
//
//   fmd_fpmatch_index_config idx; fmd_fpmatch_index_default_config(&idx);
//   fmd_host::FingerprintMatcher_GPU fm(cfg, idx);
//   fm.Update(); fm.IndexStatus(c).candidates;
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class FingerprintMatcher_GPU {
    fmd_fpmatch h = nullptr;
    fmd_fpmatch_config cfg{};
    fmd_fpmatch_index_config idx{};
    bool indexed = false;
    long long max_events = 0;
    fmd_fpmatch_event* d_events = nullptr;   // [C][max_events]
    int* d_counts = nullptr;                 // [C]
    uint8_t* d_flags = nullptr;              // [C]
    uint8_t* d_ok = nullptr;                 // [C]
    std::vector<fmd_fpmatch_status> status;
    std::vector<fmd_fpmatch_index_status> index_status;   // of an indexed object
    std::vector<int> counts;
    std::vector<uint8_t> flags;
    std::vector<fmd_fpmatch_event> events;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_fpmatch_last_error(h)); }
    void release() {
        if (h) fmd_fpmatch_destroy(h);
        for (void* p : {(void*)d_events, (void*)d_counts, (void*)d_flags, (void*)d_ok})
            if (p) (void)hipFree(p);
        h = nullptr; d_events = nullptr; d_counts = nullptr; d_flags = nullptr; d_ok = nullptr;
    }
    void create() {
        if (fmd_fpmatch_create_ex(&cfg, indexed ? &idx : nullptr, &h) != FMD_OK) throw std::runtime_error(std::string("fmd_fpmatch_create: ") + fmd_fpmatch_last_error(nullptr));
        max_events = fmd_fpmatch_max_events(cfg.interval, cfg.max_words);
        const size_t C = (size_t)cfg.n_channels;
        status.resize(C); index_status.assign(indexed ? C : 0, fmd_fpmatch_index_status{}); counts.assign(C, 0); flags.assign(C, 0); events.assign(C * (size_t)max_events, fmd_fpmatch_event{});
        // (create has made `device` current where one was given); before the first Process every count and byte is 0
        if (hipMalloc(reinterpret_cast<void**>(&d_events), sizeof(fmd_fpmatch_event) * events.size()) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&d_counts), sizeof(int) * C) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&d_flags), C) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&d_ok), C) != hipSuccess || hipMemset(d_events, 0, sizeof(fmd_fpmatch_event) * events.size()) != hipSuccess ||
            hipMemset(d_counts, 0, sizeof(int) * C) != hipSuccess || hipMemset(d_flags, 0, C) != hipSuccess || hipMemset(d_ok, 0, C) != hipSuccess) {
            release();
            throw std::runtime_error("FingerprintMatcher_GPU: the output's allocation failed");
        }
    }
public:
    explicit FingerprintMatcher_GPU(const fmd_fpmatch_config& _cfg) : cfg(_cfg) { create(); }
    // an indexed object: the catalogue is searched through its index (max_bucket, follow)
    FingerprintMatcher_GPU(const fmd_fpmatch_config& _cfg, const fmd_fpmatch_index_config& _idx) : cfg(_cfg), idx(_idx), indexed(true) { create(); }
    ~FingerprintMatcher_GPU() { release(); }
    FingerprintMatcher_GPU(const FingerprintMatcher_GPU&) = delete;
    FingerprintMatcher_GPU& operator=(const FingerprintMatcher_GPU&) = delete;

    int GetTotalChannels() const { return cfg.n_channels; }
    const fmd_fpmatch_config& Config() const { return cfg; }
    long long MaxEvents() const { return max_events; }       // events a station's view holds: also the stride from one station to the next
    bool Indexed() const { return indexed; }
    const fmd_fpmatch_index_config& IndexConfig() const { return idx; }
    long long StateBytes() const { return indexed ? fmd_fpmatch_index_state_bytes(&cfg, &idx) : fmd_fpmatch_state_bytes(&cfg); }

    // replaces the catalogue: track t is words[starts[t] ... starts[t + 1] - 1]; waits for the object's work
    void Load(const uint32_t* words, const long long* starts, int n_tracks) { check(fmd_fpmatch_load(h, words, starts, n_tracks), "fmd_fpmatch_load"); }
    void Load(const std::vector<std::vector<uint32_t>>& tracks) {
        std::vector<uint32_t> words;
        std::vector<long long> starts(1, 0);
        for (const auto& t : tracks) { words.insert(words.end(), t.begin(), t.end()); starts.push_back((long long)words.size()); }
        Load(words.data(), starts.data(), (int)tracks.size());
    }
    // takes up to n <= max_words words of every station whose d_active byte is not 0 (NULL: all): d_nwords[c] of them (NULL: n) from
    // d_words + c * words_stride; asynchronous on `stream`
    void Process(const uint32_t* d_words, long long words_stride, const int* d_nwords, int n, const unsigned char* d_active = nullptr, void* stream = nullptr) {
        check(fmd_fpmatch_process_dev(h, d_words, words_stride, d_nwords, n, d_active, d_events, max_events, d_counts, d_flags, d_ok, stream), "fmd_fpmatch_process_dev");
    }
    void Reset(int channel = -1) { check(fmd_fpmatch_reset(h, channel), "fmd_fpmatch_reset"); }

    // the device's views, written behind every Process on its stream
    const fmd_fpmatch_event* EventsDev(int c) const { return d_events + (size_t)c * (size_t)max_events; }
    const int* CountsDev() const { return d_counts; }
    const uint8_t* FlagsDev() const { return d_flags; }      // bit 0 = identified, bit 1 = the last query was a hit
    const uint8_t* OkDev() const { return d_ok; }            // 1 = identified: a gate for a recorder or a mixer bus
    const fmd_fpmatch_status* StatusDev() const {
        const fmd_fpmatch_status* p = nullptr;
        check(fmd_fpmatch_status_dev(h, &p), "fmd_fpmatch_status_dev");
        return p;
    }

    // waits for the object's work and copies every station's record, count, byte and events to the host
    void Update() {
        check(fmd_fpmatch_get_status(h, status.data()), "fmd_fpmatch_get_status");
        if (indexed) check(fmd_fpmatch_get_index_status(h, index_status.data()), "fmd_fpmatch_get_index_status");
        if (hipMemcpy(counts.data(), d_counts, sizeof(int) * counts.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(flags.data(), d_flags, flags.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(events.data(), d_events, sizeof(fmd_fpmatch_event) * events.size(), hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error("FingerprintMatcher_GPU: the output's copy failed");
    }
    // as of the last Update()
    const fmd_fpmatch_status& Status(int c) const { return status.at((size_t)c); }
    // of an indexed object (std::out_of_range otherwise)
    const fmd_fpmatch_index_status& IndexStatus(int c) const { return index_status.at((size_t)c); }
    int Events(int c) const { return counts.at((size_t)c); }
    bool Identified(int c) const { return (flags.at((size_t)c) & 1u) != 0; }
    const fmd_fpmatch_event& Event(int c, int i) const {
        if (i < 0 || i >= Events(c)) throw std::out_of_range("FingerprintMatcher_GPU::Event");
        return events[(size_t)c * (size_t)max_events + (size_t)i];
    }
    // errs as a bit error rate: compare with the paper's 0.35
    double BitErrorRate(unsigned errs) const { return (double)errs / ((double)cfg.block * (double)cfg.n_bits); }
};

}  // namespace fmd_host
