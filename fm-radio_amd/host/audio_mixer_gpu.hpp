// Header-only C++ host adaptor over the C ABI's batched audio mixer (include/fmdemod.h "Batched audio mixer") with the reference's
// mixer interface, so code written against williamyang98/FM-Radio's AudioMixer can mix every bus on the GPU:
//
//   reference (src/audio/audio_mixer.h:11-25)                    this adaptor
//   AudioMixer(int block_size)                                   AudioMixer_GPU(n_channels[, n_buses, device]): n_buses mixers over
//                                                                the rows of one device audio array
//   shared_ptr<RingBuffer> CreateManagedBuffer(int nb_blocks)    AddSource(bus, station): the station's row joins the bus, in
//                                                                registration order (the ring buffer is the caller's business)
//   float& GetOutputGain()                                       float& GetOutputGain(bus = 0)
//   span<Frame<float>> UpdateMixer()                             UpdateMixer(d_in, in_stride, n[, d_active, stream]): every bus's n
//                                                                frames in host memory (Bus(b)), or UpdateMixer(..., d_out, out_stride,
//                                                                stream) straight into device memory, asynchronously
//
// Source and gain changes apply at the next UpdateMixer.  d_active ([C] uint8 on the device, NULL = all) says which stations delivered a
// block this call: the reference counts only the ring buffers that held one.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class AudioMixer_GPU {
    fmd_mixer m = nullptr;
    int n_channels, n_buses;
    std::vector<std::vector<int>> sources;
    std::vector<bool> sources_dirty;
    std::vector<float> gains, applied_gains;
    std::vector<float> host;
    long long host_frames = 0;
    void check(int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_mixer_last_error(m)); }
    void apply() {
        for (int b = 0; b < n_buses; b++) {
            if (sources_dirty[b]) {
                check(fmd_mixer_set_sources(m, b, sources[b].data(), (int)sources[b].size()), "fmd_mixer_set_sources");
                sources_dirty[b] = false;
            }
            if (gains[b] != applied_gains[b]) {
                check(fmd_mixer_set_gain(m, b, gains[b]), "fmd_mixer_set_gain");
                applied_gains[b] = gains[b];
            }
        }
    }
public:
    explicit AudioMixer_GPU(int _n_channels, int _n_buses = 1, int device = -1)
        : n_channels(_n_channels), n_buses(_n_buses), sources(_n_buses), sources_dirty(_n_buses, false), gains(_n_buses, 1.0f),
          applied_gains(_n_buses, 1.0f) {
        std::vector<int> offsets((size_t)(_n_buses > 0 ? _n_buses : 0) + 1, 0);
        fmd_mixer_config cfg{_n_channels, _n_buses, offsets.data(), nullptr, nullptr, device};
        if (fmd_mixer_create(&cfg, &m) != FMD_OK) throw std::runtime_error(std::string("fmd_mixer_create: ") + fmd_mixer_last_error(nullptr));
    }
    ~AudioMixer_GPU() { if (m) fmd_mixer_destroy(m); }
    AudioMixer_GPU(const AudioMixer_GPU&) = delete;
    AudioMixer_GPU& operator=(const AudioMixer_GPU&) = delete;

    int GetTotalBuses() const { return n_buses; }

    // AudioMixer::CreateManagedBuffer (audio_mixer.cpp:13-19): station `station`'s audio joins bus `bus` after its earlier sources
    void AddSource(int bus, int station) {
        if (bus < 0 || bus >= n_buses || station < 0 || station >= n_channels) throw std::out_of_range("AddSource: bus or station out of range");
        sources.at((size_t)bus).push_back(station);
        sources_dirty[(size_t)bus] = true;
    }
    // AudioMixer::GetOutputGain (audio_mixer.h:24)
    float& GetOutputGain(int bus = 0) { return gains.at((size_t)bus); }

    // AudioMixer::UpdateMixer (audio_mixer.cpp:33-79) for every bus, delivered to host memory after `stream` has finished:
    // bus b's n frames (interleaved L, R) are Bus(b)
    long long UpdateMixer(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        apply();
        host.resize((size_t)n_buses * (size_t)(n > 0 ? n : 1) * 2);
        check(fmd_mixer_process_f32_host(m, d_in, in_stride, n, d_active, host.data(), n > 0 ? n : 1, stream), "fmd_mixer_process_f32_host");
        host_frames = n;
        return n;
    }
    const float* Bus(int b) const { return host.data() + (size_t)b * (size_t)(host_frames > 0 ? host_frames : 1) * 2; }
    long long GetFrames() const { return host_frames; }

    // device to device, asynchronous on `stream`: d_out [n_buses][out_stride][2]
    void UpdateMixer(const float* d_in, long long in_stride, long long n, const uint8_t* d_active, float* d_out, long long out_stride, void* stream) {
        apply();
        check(fmd_mixer_process_f32_dev(m, d_in, in_stride, n, d_active, d_out, out_stride, stream), "fmd_mixer_process_f32_dev");
    }
};

}  // namespace fmd_host
