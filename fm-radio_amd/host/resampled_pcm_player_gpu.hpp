// Header-only C++ host adaptor over the C ABI's batched audio resampler (include/fmdemod.h "Batched audio resampler") with the
// reference's player interface, so code written against williamyang98/FM-Radio's Resampled_PCM_Player can resample every station on
// the GPU:
//
//   reference (src/audio/resampled_pcm_player.h:9-20)            this adaptor
//   Resampled_PCM_Player(buffer, int output_sample_rate)          Resampled_PCM_Player_GPU(n_channels, output_sample_rate[, method, ...])
//   void ConsumeBuffer(span<const Frame<float>>)                  ConsumeBuffer(d_frames, in_stride, n, stream): device frames of every
//                                                                 channel (fmd_audio_dev's view: in_stride = n_audio) -> OnAudioOut
//                                                                 observers (host frames at the output rate, one call per channel), or
//                                                                 ConsumeBuffer(d_frames, in_stride, n, d_out, out_stride, stream) /
//                                                                 ConsumeBufferPCM16(...) straight into device memory, asynchronously
//   bool SetInputSampleRate(int)                                  bool SetInputSampleRate(int)
//
// The reference hands the resampled block to a ring buffer feeding PortAudio; here an observer takes it (an Audio_WAV_Writer of
// fm_scraper_writer.hpp opened at GetOutputSampleRate(), a network sink, ...).
#pragma once

#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class Resampled_PCM_Player_GPU {
    fmd_resampler r = nullptr;
    int n_channels, output_sample_rate, input_sample_rate;
    std::vector<float> host;
    std::vector<std::function<void(int, const float*, size_t, int)>> observers;
    void check(int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_resampler_last_error(r)); }
public:
    Resampled_PCM_Player_GPU(int _n_channels, int _output_sample_rate, int method = FMD_RESAMPLE_POLYPHASE, long long max_input_frames = 65536,
                             int _input_sample_rate = 32000, int device = -1)
        : n_channels(_n_channels), output_sample_rate(_output_sample_rate), input_sample_rate(_input_sample_rate) {
        fmd_resampler_config cfg{_n_channels, _input_sample_rate, _output_sample_rate, method, 0, max_input_frames, device};
        if (fmd_resampler_create(&cfg, &r) != FMD_OK) throw std::runtime_error(std::string("fmd_resampler_create: ") + fmd_resampler_last_error(nullptr));
    }
    ~Resampled_PCM_Player_GPU() { if (r) fmd_resampler_destroy(r); }
    Resampled_PCM_Player_GPU(const Resampled_PCM_Player_GPU&) = delete;
    Resampled_PCM_Player_GPU& operator=(const Resampled_PCM_Player_GPU&) = delete;

    int GetOutputSampleRate() const { return output_sample_rate; }
    int GetInputSampleRate() const { return input_sample_rate; }
    // frames per channel the next ConsumeBuffer of n input frames delivers
    long long GetOutputFrames(long long n) { long long o = 0; check(fmd_resampler_output_frames(r, n, &o), "fmd_resampler_output_frames"); return o; }

    // Resampled_PCM_Player::SetInputSampleRate (resampled_pcm_player.cpp:29-33)
    bool SetInputSampleRate(int fs) {
        const int rc = fmd_resampler_set_input_rate(r, fs);
        check(rc, "fmd_resampler_set_input_rate");
        input_sample_rate = fs;
        return rc == 1;
    }
    void Reset(int channel = -1) { check(fmd_resampler_reset(r, channel), "fmd_resampler_reset"); }

    // observers of the resampled host frames: (channel, interleaved L,R frames, n_frames, output rate)
    void OnAudioOut(const std::function<void(int, const float*, size_t, int)>& fn) { observers.push_back(fn); }

    // Resampled_PCM_Player::ConsumeBuffer (resampled_pcm_player.cpp:15-27) for every channel, delivered to the observers on the caller's
    // thread after `stream` has finished the block (fmd_resampler_process_f32_host)
    long long ConsumeBuffer(const float* d_frames, long long in_stride, long long n, void* stream = nullptr) {
        const long long want = GetOutputFrames(n);
        host.resize((size_t)n_channels * (size_t)(want > 0 ? want : 1) * 2);
        long long got = 0;
        check(fmd_resampler_process_f32_host(r, d_frames, in_stride, n, host.data(), want > 0 ? want : 1, &got, stream), "fmd_resampler_process_f32_host");
        for (int c = 0; c < n_channels; c++)
            for (auto& o : observers) o(c, host.data() + (size_t)c * (size_t)(want > 0 ? want : 1) * 2, (size_t)got, output_sample_rate);
        return got;
    }
    // device to device, asynchronous on `stream`: d_out [C][out_stride][2]
    long long ConsumeBuffer(const float* d_frames, long long in_stride, long long n, float* d_out, long long out_stride, void* stream) {
        long long got = 0;
        check(fmd_resampler_process_f32_dev(r, d_frames, in_stride, n, d_out, out_stride, &got, stream), "fmd_resampler_process_f32_dev");
        return got;
    }
    long long ConsumeBufferPCM16(const float* d_frames, long long in_stride, long long n, int16_t* d_out, long long out_stride, void* stream) {
        long long got = 0;
        check(fmd_resampler_process_pcm16_dev(r, d_frames, in_stride, n, d_out, out_stride, &got, stream), "fmd_resampler_process_pcm16_dev");
        return got;
    }
};

}  // namespace fmd_host
