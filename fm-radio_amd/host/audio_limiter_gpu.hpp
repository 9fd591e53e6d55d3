// Header-only C++ host adaptor over the C ABI's look-ahead peak limiter (include/fmdemod.h "Look-ahead peak limiter"): RAII around the
// handle and the device array it writes, exceptions instead of status codes.  NOT in the reference (williamyang98/FM-Radio ends its
// mixer in a hard clip); it reads the station audio [C][in_stride][2] f32 that the mixer, the monitors and the encoders read, or a
// mixer's bus output:
//
//   fmd_host::AudioLimiter_GPU lim(n_channels, 32000, frames_per_block);       // 1.5 ms look-ahead, 500 ms release, -1 dBFS
//   lim.SetGain(fmd_limiter_gain_for_loudness(lufs, -23.0), c);                // from the loudness meter's integrated figure
//   const float* d_y = lim.Process(d_audio, in_stride, n, d_active, stream);   // [C][OutStride()][2] f32 on the device, n frames a row
//   const float* d_t = lim.Flush(stream);                                      // the last GetLatency() frames, at a stream's end
//
// The output trails the input by GetLatency() frames.  It stays valid until the next Process or Flush.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class AudioLimiter_GPU {
    fmd_limiter l = nullptr;
    int n_channels;
    long long out_stride;                    // frames of a row of d_out
    fmd_limiter_design_t design{};
    float* d_out = nullptr;                  // [C][out_stride][2]
    float* d_gr = nullptr;                   // [C]
    std::vector<fmd_limiter_status> status;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_limiter_last_error(l)); }
    void release() {
        if (l) fmd_limiter_destroy(l);
        l = nullptr;
        if (d_out) (void)hipFree(d_out);
        if (d_gr) (void)hipFree(d_gr);
        d_out = nullptr; d_gr = nullptr;
    }
public:
    AudioLimiter_GPU(int _n_channels, int fs, long long max_input_frames, double lookahead_ms = 1.5, double release_ms = 500.0, double ceiling_db = -1.0,
                     int device = -1)
        : n_channels(_n_channels), out_stride(0) {
        fmd_limiter_config cfg{_n_channels, fs, lookahead_ms, release_ms, ceiling_db, max_input_frames, device};
        if (fmd_limiter_create(&cfg, &l) != FMD_OK) throw std::runtime_error(std::string("fmd_limiter_create: ") + fmd_limiter_last_error(nullptr));
        (void)fmd_limiter_design(fs, lookahead_ms, release_ms, ceiling_db, &design);
        out_stride = max_input_frames > design.latency_frames ? max_input_frames : design.latency_frames;
        const size_t C = (size_t)n_channels;
        status.resize(C);
        // (create has made `device` current where one was given)
        if (hipMalloc(reinterpret_cast<void**>(&d_out), sizeof(float) * 2 * C * (size_t)out_stride) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&d_gr), sizeof(float) * C) != hipSuccess) {
            release();
            throw std::runtime_error("AudioLimiter_GPU: the outputs' allocation failed");
        }
    }
    ~AudioLimiter_GPU() { release(); }
    AudioLimiter_GPU(const AudioLimiter_GPU&) = delete;
    AudioLimiter_GPU& operator=(const AudioLimiter_GPU&) = delete;

    int GetTotalChannels() const { return n_channels; }
    int GetLatency() const { return design.latency_frames; }
    float GetCeiling() const { return design.ceiling; }
    long long OutStride() const { return out_stride; }

    // channel -1: every station
    void SetGain(float gain, int channel = -1) { check(fmd_limiter_set_gain(l, channel, gain), "fmd_limiter_set_gain"); }
    float GetGain(int channel) const {
        float g = 0.0f;
        check(fmd_limiter_get_gain(l, channel, &g), "fmd_limiter_get_gain");
        return g;
    }
    void Reset(int channel = -1) { check(fmd_limiter_reset(l, channel), "fmd_limiter_reset"); }

    // takes n frames of every station whose d_active byte is not 0 (NULL: all); returns the device output, n frames a row, asynchronous
    // on `stream`
    const float* Process(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        check(fmd_limiter_process_f32_dev(l, d_in, in_stride, n, d_active, d_out, out_stride, d_gr, stream), "fmd_limiter_process_f32_dev");
        return d_out;
    }
    // each station's smallest gain over the last Process, [C] f32 on the device
    const float* GainReductionDev() const { return d_gr; }
    // the GetLatency() frames that as many frames of silence push out, a row; the stations stand as after Reset, counters and gains kept
    const float* Flush(void* stream = nullptr) {
        check(fmd_limiter_flush(l, -1, d_out, out_stride, nullptr, stream), "fmd_limiter_flush");
        return d_out;
    }
    // waits for the limiter's work and copies every station's record to the host
    void Update() { check(fmd_limiter_get_status(l, status.data()), "fmd_limiter_get_status"); }
    // as of the last Update()
    const fmd_limiter_status& Status(int c) const { return status.at((size_t)c); }
    // the device's own records, for a consumer on the device (valid until the next Process)
    const fmd_limiter_status* StatusDev() const {
        const fmd_limiter_status* p = nullptr;
        check(fmd_limiter_status_dev(l, &p), "fmd_limiter_status_dev");
        return p;
    }
};

}  // namespace fmd_host
