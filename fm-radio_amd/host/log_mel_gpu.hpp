// Header-only C++ host adaptor over the C ABI's log-mel front end (include/fmdemod.h "Log-mel front end"): RAII around the handle, the
// output tensor [C][max_frames][n_mels] f32 for a given max_input_frames and the [C] counts on the device, exceptions instead of status
// codes, and per-station views.  NOT in the reference (williamyang98/FM-Radio plays one station to a listener): it reads the station audio
// [C][in_stride][2] f32 that the mixer and the monitors read, and what it writes is a model's input:
//
//   fmd_host::LogMel_GPU mel(n_channels, 32000, frames_per_block);     // the default geometry: 800 / 320 / 80 bands, log10
//   mel.Process(d_audio, in_stride, n, nullptr, stream);               // asynchronous on the stream given
//   model.Forward(mel.RowsDev(c), mel.CountsDev(), ...);               // on the device, no host round trip
//   mel.Update();                                                      // or: waits, copies counts, records and rows to the host
//   mel.Frames(c); mel.Row(c, t)[band]; mel.FrameTime(c, t);
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class LogMel_GPU {
    fmd_logmel h = nullptr;
    fmd_logmel_config cfg{};
    long long max_frames = 0, out_stride = 0;
    float* d_out = nullptr;                  // [C][max_frames][n_mels]
    int* d_counts = nullptr;                 // [C]
    std::vector<fmd_logmel_status> status;
    std::vector<int> counts;
    std::vector<float> rows;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_logmel_last_error(h)); }
    void init() {
        if (fmd_logmel_create(&cfg, &h) != FMD_OK) throw std::runtime_error(std::string("fmd_logmel_create: ") + fmd_logmel_last_error(nullptr));
        max_frames = fmd_logmel_max_frames(cfg.hop, cfg.max_input_frames);
        out_stride = max_frames * (long long)cfg.n_mels;
        const size_t C = (size_t)cfg.n_channels;
        status.resize(C); counts.assign(C, 0); rows.assign(C * (size_t)out_stride, 0.0f);
        // (create has made `device` current where one was given); before the first Process every count is 0
        if (hipMalloc(reinterpret_cast<void**>(&d_out), sizeof(float) * rows.size()) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&d_counts), sizeof(int) * C) != hipSuccess ||
            hipMemset(d_out, 0, sizeof(float) * rows.size()) != hipSuccess || hipMemset(d_counts, 0, sizeof(int) * C) != hipSuccess) {
            release();
            throw std::runtime_error("LogMel_GPU: the output's allocation failed");
        }
    }
    void release() {
        if (h) fmd_logmel_destroy(h);
        if (d_out) (void)hipFree(d_out);
        if (d_counts) (void)hipFree(d_counts);
        h = nullptr; d_out = nullptr; d_counts = nullptr;
    }
public:
    // the default geometry at the audio's own rate
    LogMel_GPU(int n_channels, int fs, long long max_input_frames, int device = -1) {
        if (fmd_logmel_default_config(fs, &cfg) != FMD_OK) throw std::runtime_error(std::string("fmd_logmel_default_config: ") + fmd_logmel_last_error(nullptr));
        cfg.n_channels = n_channels; cfg.max_input_frames = max_input_frames; cfg.device = device;
        init();
    }
    explicit LogMel_GPU(const fmd_logmel_config& _cfg) : cfg(_cfg) { init(); }
    ~LogMel_GPU() { release(); }
    LogMel_GPU(const LogMel_GPU&) = delete;
    LogMel_GPU& operator=(const LogMel_GPU&) = delete;

    int GetTotalChannels() const { return cfg.n_channels; }
    const fmd_logmel_config& Config() const { return cfg; }
    long long MaxFrames() const { return max_frames; }       // rows a station's view holds
    long long OutStride() const { return out_stride; }       // floats from one station's rows to the next's

    // takes n <= max_input_frames frames of every station whose d_active byte is not 0 (NULL: all); asynchronous on `stream`
    void Process(const float* d_in, long long in_stride, long long n, const unsigned char* d_active = nullptr, void* stream = nullptr) {
        check(fmd_logmel_process_f32_dev(h, d_in, in_stride, n, d_active, d_out, out_stride, d_counts, stream), "fmd_logmel_process_f32_dev");
    }
    void Reset(int channel = -1) { check(fmd_logmel_reset(h, channel), "fmd_logmel_reset"); }

    // the device's views, written behind every Process on its stream: station c's rows [MaxFrames()][n_mels], of which the first
    // CountsDev()[c] are the last call's
    const float* RowsDev(int c) const { return d_out + (size_t)c * (size_t)out_stride; }
    const int* CountsDev() const { return d_counts; }
    const fmd_logmel_status* StatusDev() const {
        const fmd_logmel_status* p = nullptr;
        check(fmd_logmel_status_dev(h, &p), "fmd_logmel_status_dev");
        return p;
    }

    // waits for the object's work and copies every station's record, count and rows to the host
    void Update() {
        check(fmd_logmel_get_status(h, status.data()), "fmd_logmel_get_status");
        if (hipMemcpy(counts.data(), d_counts, sizeof(int) * counts.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(rows.data(), d_out, sizeof(float) * rows.size(), hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error("LogMel_GPU: the output's copy failed");
    }
    // as of the last Update()
    const fmd_logmel_status& Status(int c) const { return status.at((size_t)c); }
    int Frames(int c) const { return counts.at((size_t)c); }
    const float* Row(int c, int t) const {
        if (t < 0 || t >= Frames(c)) throw std::out_of_range("LogMel_GPU::Row");
        return rows.data() + (size_t)c * (size_t)out_stride + (size_t)t * (size_t)cfg.n_mels;
    }
    // the centre of row t of the last call in seconds since the station's reset
    double FrameTime(int c, int t) const {
        const unsigned long long first = Status(c).spectra - (unsigned long long)Frames(c);
        return ((double)(first + (unsigned long long)t) * (double)cfg.hop + 0.5 * (double)cfg.win) / (double)cfg.fs;
    }
};

}  // namespace fmd_host
