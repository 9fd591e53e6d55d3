// Header-only C++ host adaptor over the C ABI's audio fault monitor (include/fmdemod.h "Audio fault monitor"): RAII around the handle
// and the two device byte arrays it writes, exceptions instead of status codes, and the read-outs in dB.  NOT in the reference
// (williamyang98/FM-Radio plays one station to a listener): it reads the station audio [C][in_stride][2] f32 that the resampler, the
// mixer and the loudness meter read, and its ok bytes are what the mixer takes as d_active:
//
//   fmd_host::AudioMonitor_GPU mon(n_channels, 32000, frames_per_block);
//   mon.Process(d_audio, in_stride, n, nullptr, stream);               // asynchronous on the stream given
//   mixer.Process(..., mon.OkDev(), stream);                           // a dead or antiphase station leaves the bus: no host round trip
//   mon.Update();                                                      // waits, reads 840 bytes and the two bytes per station
//   mon.Flags(c) & FMD_AUDMON_SILENCE; mon.IsOk(c); mon.LevelDb(c, 2, 10); mon.Correlation(c, 10);
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class AudioMonitor_GPU {
    fmd_audmon a = nullptr;
    int n_channels, fs;
    uint8_t* d_bytes = nullptr;              // [2][C]: flags, ok
    std::vector<fmd_audmon_status> status;
    std::vector<uint8_t> bytes;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_audmon_last_error(a)); }
    static double nan() { return std::numeric_limits<double>::quiet_NaN(); }
public:
    AudioMonitor_GPU(int _n_channels, int _fs, long long max_input_frames, int device = -1)
        : n_channels(_n_channels), fs(_fs), status((size_t)(_n_channels > 0 ? _n_channels : 0)), bytes(2 * (size_t)(_n_channels > 0 ? _n_channels : 0)) {
        fmd_audmon_config cfg{_n_channels, _fs, max_input_frames, device};
        if (fmd_audmon_create(&cfg, &a) != FMD_OK) throw std::runtime_error(std::string("fmd_audmon_create: ") + fmd_audmon_last_error(nullptr));
        // (create has made `device` current where one was given); before the first Process every flag is clear and every station ok
        if (hipMalloc(reinterpret_cast<void**>(&d_bytes), bytes.size()) != hipSuccess || hipMemset(d_bytes, 0, status.size()) != hipSuccess ||
            hipMemset(d_bytes + status.size(), 1, status.size()) != hipSuccess) {
            fmd_audmon_destroy(a);
            throw std::runtime_error("AudioMonitor_GPU: the bytes' allocation failed");
        }
    }
    ~AudioMonitor_GPU() {
        if (a) fmd_audmon_destroy(a);
        if (d_bytes) (void)hipFree(d_bytes);
    }
    AudioMonitor_GPU(const AudioMonitor_GPU&) = delete;
    AudioMonitor_GPU& operator=(const AudioMonitor_GPU&) = delete;

    int GetTotalChannels() const { return n_channels; }
    // the [C] uint8 arrays on the device, written behind every Process on its stream; OkDev() is another object's d_active
    const uint8_t* FlagsDev() const { return d_bytes; }
    const uint8_t* OkDev() const { return d_bytes + status.size(); }

    // takes n frames of every station whose d_active byte is not 0 (NULL: all) and writes their two bytes; asynchronous on `stream`
    void Process(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        check(fmd_audmon_process_f32_dev(a, d_in, in_stride, n, d_active, d_bytes, d_bytes + status.size(), stream), "fmd_audmon_process_f32_dev");
    }
    void Reset(int channel = -1) { check(fmd_audmon_reset(a, channel), "fmd_audmon_reset"); }
    void ResetPeaks(int channel = -1) { check(fmd_audmon_reset_peaks(a, channel), "fmd_audmon_reset_peaks"); }
    void SetParams(const fmd_audmon_params& p, int channel = -1) { check(fmd_audmon_set_params(a, channel, &p), "fmd_audmon_set_params"); }
    fmd_audmon_params GetParams(int channel) const {
        fmd_audmon_params p;
        check(fmd_audmon_get_params(a, channel, &p), "fmd_audmon_get_params");
        return p;
    }

    // waits for the monitor's work and copies every station's record and two bytes to the host
    void Update() {
        check(fmd_audmon_get_status(a, status.data()), "fmd_audmon_get_status");
        if (hipMemcpy(bytes.data(), d_bytes, bytes.size(), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("AudioMonitor_GPU: the bytes' copy failed");
    }
    // as of the last Update()
    const fmd_audmon_status& Status(int c) const { return status.at((size_t)c); }
    unsigned Flags(int c) const { return bytes.at((size_t)c); }
    bool IsOk(int c) const { return bytes.at(status.size() + (size_t)c) != 0; }
    // NaN while fewer than `window` intervals are complete (and where the figure itself is 0 / 0)
    double LevelDb(int c, int rail = 2, int window = 1) const { double v = 0.0; return fmd_audmon_level_db(&Status(c), fs, rail, window, &v) == FMD_OK ? v : nan(); }
    double BalanceDb(int c, int window = 1) const { double v = 0.0; return fmd_audmon_balance_db(&Status(c), fs, window, &v) == FMD_OK ? v : nan(); }
    double Correlation(int c, int window = 1) const { double v = 0.0; return fmd_audmon_correlation(&Status(c), fs, window, &v) == FMD_OK ? v : nan(); }
    double SideMidDb(int c, int window = 1) const { double v = 0.0; return fmd_audmon_side_mid_db(&Status(c), fs, window, &v) == FMD_OK ? v : nan(); }
    // the device's own records, for a consumer on the device (valid until the next Process)
    const fmd_audmon_status* StatusDev() const {
        const fmd_audmon_status* p = nullptr;
        check(fmd_audmon_status_dev(a, &p), "fmd_audmon_status_dev");
        return p;
    }
};

}  // namespace fmd_host
