// Header-only C++ host adaptor over the C ABI's DC offset and IQ imbalance corrector (include/fmdemod.h "DC offset and IQ imbalance
// correction"): an RAII handle with exceptions for errors.  The reference has no counterpart (its RTL-SDR hardware is low-IF), so the
// interface is the C ABI's own:
//
//   IqCorrector_GPU corr(max_input_samples[, device]);
//   corr.Measure(d_block, n, stream);            // first block(s): moments only
//   corr.Calibrate();                            // solve and adopt the correction
//   corr.Process(d_block, n, d_cf32, stream);    // every block, ahead of fmd_scan_process_* / fmd_chan_process_*
//
// Process and Measure are overloaded on the sample type: float (cf32), uint8_t, int8_t, int16_t.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>

#include "fmdemod.h"

namespace fmd_host {

class IqCorrector_GPU {
    fmd_iqcorr h = nullptr;
    void check(int rc, const char* what) { if (rc != FMD_OK) throw std::runtime_error(std::string(what) + ": " + fmd_iqcorr_last_error(h)); }
public:
    explicit IqCorrector_GPU(long long max_input_samples, int device = -1) {
        fmd_iqcorr_config cfg{max_input_samples, device};
        if (fmd_iqcorr_create(&cfg, &h) != FMD_OK) throw std::runtime_error(std::string("fmd_iqcorr_create: ") + fmd_iqcorr_last_error(nullptr));
    }
    ~IqCorrector_GPU() { if (h) fmd_iqcorr_destroy(h); }
    IqCorrector_GPU(const IqCorrector_GPU&) = delete;
    IqCorrector_GPU& operator=(const IqCorrector_GPU&) = delete;

    // d_in [n][2] on the device -> d_out [n][2] cf32 on the device (d_out == d_in allowed for cf32), asynchronous on `stream`
    void Process(const float* d_in, long long n, float* d_out, void* stream = nullptr) { check(fmd_iqcorr_process_cf32_dev(h, d_in, n, d_out, stream), "fmd_iqcorr_process_cf32_dev"); }
    void Process(const uint8_t* d_in, long long n, float* d_out, void* stream = nullptr) { check(fmd_iqcorr_process_u8_dev(h, d_in, n, d_out, stream), "fmd_iqcorr_process_u8_dev"); }
    void Process(const int8_t* d_in, long long n, float* d_out, void* stream = nullptr) { check(fmd_iqcorr_process_s8_dev(h, d_in, n, d_out, stream), "fmd_iqcorr_process_s8_dev"); }
    void Process(const int16_t* d_in, long long n, float* d_out, void* stream = nullptr) { check(fmd_iqcorr_process_s16_dev(h, d_in, n, d_out, stream), "fmd_iqcorr_process_s16_dev"); }
    // moments only
    template <typename T> void Measure(const T* d_in, long long n, void* stream = nullptr) { Process(d_in, n, nullptr, stream); }

    fmd_iq_moments GetMoments() { fmd_iq_moments m{}; check(fmd_iqcorr_get_moments(h, &m), "fmd_iqcorr_get_moments"); return m; }
    // the solve step: host only, needs no corrector
    static fmd_iq_correction Solve(const fmd_iq_moments& m) {
        fmd_iq_correction c{};
        if (fmd_iqcorr_solve(&m, &c) != FMD_OK) throw std::runtime_error(std::string("fmd_iqcorr_solve: ") + fmd_iqcorr_last_error(nullptr));
        return c;
    }
    // GetMoments, Solve, SetCorrection; the moments are kept
    fmd_iq_correction Calibrate() { fmd_iq_correction c{}; check(fmd_iqcorr_calibrate(h, &c), "fmd_iqcorr_calibrate"); return c; }
    void SetCorrection(const fmd_iq_correction& c) { check(fmd_iqcorr_set_correction(h, &c), "fmd_iqcorr_set_correction"); }
    fmd_iq_correction GetCorrection() { fmd_iq_correction c{}; check(fmd_iqcorr_get_correction(h, &c), "fmd_iqcorr_get_correction"); return c; }
    void Reset() { check(fmd_iqcorr_reset(h), "fmd_iqcorr_reset"); }
    void ResetMoments() { check(fmd_iqcorr_reset_moments(h), "fmd_iqcorr_reset_moments"); }
};

}  // namespace fmd_host
