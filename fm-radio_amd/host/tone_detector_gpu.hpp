// Header-only C++ host adaptor over the C ABI's audio tone detector (include/fmdemod.h "Audio tone detector"): RAII around the handle
// and the two device byte arrays it writes, exceptions instead of status codes, and the read-outs in dB.  NOT in the reference
// (williamyang98/FM-Radio plays one station to a listener): it reads the station audio [C][in_stride][2] f32 that the mixer, the
// loudness meter and the fault monitor read, and its ok bytes are what the mixer takes as d_active:
//
//   fmd_host::ToneDetector_GPU det(n_channels, 32000, frames_per_block);
//   det.Process(d_audio, in_stride, n, nullptr, stream);               // asynchronous on the stream given
//   mixer.Process(..., det.OkDev(), stream);                           // a station on line-up tone leaves the bus: no host round trip
//   det.Update();                                                      // waits, reads 2344 bytes and the two bytes per station
//   det.Flags(c) & (1u << slot); det.IsOk(c); det.ShareDb(c, slot, 10); det.LevelDb(c, slot, 10);
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class ToneDetector_GPU {
    fmd_tonedet t = nullptr;
    int n_channels, fs;
    uint8_t* d_bytes = nullptr;              // [2][C]: flags, ok
    std::vector<fmd_tonedet_status> status;
    std::vector<uint8_t> bytes;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_tonedet_last_error(t)); }
    static double nan() { return std::numeric_limits<double>::quiet_NaN(); }
public:
    ToneDetector_GPU(int _n_channels, int _fs, long long max_input_frames, int device = -1)
        : n_channels(_n_channels), fs(_fs), status((size_t)(_n_channels > 0 ? _n_channels : 0)), bytes(2 * (size_t)(_n_channels > 0 ? _n_channels : 0)) {
        fmd_tonedet_config cfg{_n_channels, _fs, max_input_frames, device};
        if (fmd_tonedet_create(&cfg, &t) != FMD_OK) throw std::runtime_error(std::string("fmd_tonedet_create: ") + fmd_tonedet_last_error(nullptr));
        // (create has made `device` current where one was given); before the first Process every flag is clear and every station ok
        if (hipMalloc(reinterpret_cast<void**>(&d_bytes), bytes.size()) != hipSuccess || hipMemset(d_bytes, 0, status.size()) != hipSuccess ||
            hipMemset(d_bytes + status.size(), 1, status.size()) != hipSuccess) {
            fmd_tonedet_destroy(t);
            throw std::runtime_error("ToneDetector_GPU: the bytes' allocation failed");
        }
    }
    ~ToneDetector_GPU() {
        if (t) fmd_tonedet_destroy(t);
        if (d_bytes) (void)hipFree(d_bytes);
    }
    ToneDetector_GPU(const ToneDetector_GPU&) = delete;
    ToneDetector_GPU& operator=(const ToneDetector_GPU&) = delete;

    int GetTotalChannels() const { return n_channels; }
    // the [C] uint8 arrays on the device, written behind every Process on its stream; OkDev() is another object's d_active
    const uint8_t* FlagsDev() const { return d_bytes; }
    const uint8_t* OkDev() const { return d_bytes + status.size(); }

    // takes n frames of every station whose d_active byte is not 0 (NULL: all) and writes their two bytes; asynchronous on `stream`
    void Process(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        check(fmd_tonedet_process_f32_dev(t, d_in, in_stride, n, d_active, d_bytes, d_bytes + status.size(), stream), "fmd_tonedet_process_f32_dev");
    }
    void Reset(int channel = -1) { check(fmd_tonedet_reset(t, channel), "fmd_tonedet_reset"); }
    void SetParams(const fmd_tonedet_params& p, int channel = -1) { check(fmd_tonedet_set_params(t, channel, &p), "fmd_tonedet_set_params"); }
    fmd_tonedet_params GetParams(int channel) const {
        fmd_tonedet_params p;
        check(fmd_tonedet_get_params(t, channel, &p), "fmd_tonedet_get_params");
        return p;
    }

    // waits for the detector's work and copies every station's record and two bytes to the host
    void Update() {
        check(fmd_tonedet_get_status(t, status.data()), "fmd_tonedet_get_status");
        if (hipMemcpy(bytes.data(), d_bytes, bytes.size(), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("ToneDetector_GPU: the bytes' copy failed");
    }
    // as of the last Update()
    const fmd_tonedet_status& Status(int c) const { return status.at((size_t)c); }
    unsigned Flags(int c) const { return bytes.at((size_t)c); }
    bool IsOk(int c) const { return bytes.at(status.size() + (size_t)c) != 0; }
    // NaN while fewer than `window` intervals are complete (and where the figure itself is 0 / 0)
    double ShareDb(int c, int slot, int window = 1) const { double v = 0.0; return fmd_tonedet_share_db(&Status(c), fs, slot, window, &v) == FMD_OK ? v : nan(); }
    double LevelDb(int c, int slot, int window = 1) const { double v = 0.0; return fmd_tonedet_level_db(&Status(c), fs, slot, window, &v) == FMD_OK ? v : nan(); }
    // the device's own records, for a consumer on the device (valid until the next Process)
    const fmd_tonedet_status* StatusDev() const {
        const fmd_tonedet_status* p = nullptr;
        check(fmd_tonedet_status_dev(t, &p), "fmd_tonedet_status_dev");
        return p;
    }
};

}  // namespace fmd_host
