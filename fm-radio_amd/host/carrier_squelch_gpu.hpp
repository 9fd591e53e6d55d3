// Header-only C++ host adaptor over the C ABI's carrier squelch (include/fmdemod.h "Carrier squelch"): RAII around the handle and the
// device mask it writes, exceptions instead of status codes, and the read-out in dB.  NOT in the reference (williamyang98/FM-Radio tunes
// one station in hardware): it reads the station baseband [C][in_stride][2] that the demodulator takes, cf32 or u8, and its mask is what
// the mixer, the loudness meter and the modulation monitor take as d_active:
//
//   fmd_host::CarrierSquelch_GPU sq(n_channels, 256000, block_size);
//   sq.Process(d_iq, block_size, block_size, nullptr, stream);        // asynchronous on the stream given
//   mixer.Process(..., sq.MaskDev(), stream);                          // no host round trip
//   sq.Update();                                                       // waits, reads 368 bytes and the mask byte per station
//   sq.IsOpen(c); sq.CnrDb(c, 20); sq.LevelDb(c);
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class CarrierSquelch_GPU {
    fmd_squelch q = nullptr;
    int n_channels, fs;
    uint8_t* d_mask = nullptr;
    std::vector<fmd_squelch_status> status;
    std::vector<uint8_t> mask;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_squelch_last_error(q)); }
    static double nan() { return std::numeric_limits<double>::quiet_NaN(); }
public:
    CarrierSquelch_GPU(int _n_channels, int _fs, long long max_input_samples, int device = -1)
        : n_channels(_n_channels), fs(_fs), status((size_t)(_n_channels > 0 ? _n_channels : 0)), mask((size_t)(_n_channels > 0 ? _n_channels : 0)) {
        fmd_squelch_config cfg{_n_channels, _fs, max_input_samples, device};
        if (fmd_squelch_create(&cfg, &q) != FMD_OK) throw std::runtime_error(std::string("fmd_squelch_create: ") + fmd_squelch_last_error(nullptr));
        // (create has made `device` current where one was given)
        if (hipMalloc(reinterpret_cast<void**>(&d_mask), mask.size()) != hipSuccess || hipMemset(d_mask, 0, mask.size()) != hipSuccess) {
            fmd_squelch_destroy(q);
            throw std::runtime_error("CarrierSquelch_GPU: the mask's allocation failed");
        }
    }
    ~CarrierSquelch_GPU() {
        if (q) fmd_squelch_destroy(q);
        if (d_mask) (void)hipFree(d_mask);
    }
    CarrierSquelch_GPU(const CarrierSquelch_GPU&) = delete;
    CarrierSquelch_GPU& operator=(const CarrierSquelch_GPU&) = delete;

    int GetTotalChannels() const { return n_channels; }
    // the [C] uint8 mask on the device, written behind every Process on its stream: another object's d_active
    const uint8_t* MaskDev() const { return d_mask; }

    // takes n samples of every station whose d_active byte is not 0 (NULL: all) and writes their mask bytes; asynchronous on `stream`
    void Process(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        check(fmd_squelch_process_cf32_dev(q, d_in, in_stride, n, d_active, d_mask, stream), "fmd_squelch_process_cf32_dev");
    }
    void Process(const uint8_t* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        check(fmd_squelch_process_u8_dev(q, d_in, in_stride, n, d_active, d_mask, stream), "fmd_squelch_process_u8_dev");
    }
    void Reset(int channel = -1) { check(fmd_squelch_reset(q, channel), "fmd_squelch_reset"); }
    void ResetPeaks(int channel = -1) { check(fmd_squelch_reset_peaks(q, channel), "fmd_squelch_reset_peaks"); }
    void SetParams(const fmd_squelch_params& p, int channel = -1) { check(fmd_squelch_set_params(q, channel, &p), "fmd_squelch_set_params"); }
    fmd_squelch_params GetParams(int channel) const {
        fmd_squelch_params p;
        check(fmd_squelch_get_params(q, channel, &p), "fmd_squelch_get_params");
        return p;
    }

    // waits for the squelch's work and copies every station's record and mask byte to the host
    void Update() {
        check(fmd_squelch_get_status(q, status.data()), "fmd_squelch_get_status");
        if (hipMemcpy(mask.data(), d_mask, mask.size(), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("CarrierSquelch_GPU: the mask's copy failed");
    }
    // as of the last Update()
    const fmd_squelch_status& Status(int c) const { return status.at((size_t)c); }
    bool IsOpen(int c) const { return mask.at((size_t)c) != 0; }
    // dB; NaN while fewer than `window` intervals are complete
    double LevelDb(int c) const { double v = 0.0; return fmd_squelch_level_db(&Status(c), fs, &v) == FMD_OK ? v : nan(); }
    double CnrDb(int c, int window = 1) const { double v = 0.0; return fmd_squelch_cnr_db(&Status(c), fs, window, &v) == FMD_OK ? v : nan(); }
    // the device's own records, for a consumer on the device (valid until the next Process)
    const fmd_squelch_status* StatusDev() const {
        const fmd_squelch_status* p = nullptr;
        check(fmd_squelch_status_dev(q, &p), "fmd_squelch_status_dev");
        return p;
    }
};

}  // namespace fmd_host
