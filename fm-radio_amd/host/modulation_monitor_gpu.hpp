// Header-only C++ host adaptor over the C ABI's FM modulation monitor (include/fmdemod.h "FM modulation monitor"): RAII around the
// handle, exceptions instead of status codes, and the read-out in Hz and dBr.  NOT in the reference (williamyang98/FM-Radio measures
// nothing of the transmission): it reads the station baseband [C][in_stride][2] that the demodulator takes, cf32 or u8:
//
//   fmd_host::ModulationMonitor_GPU mon(n_channels, 256000, block_size);
//   mon.Process(d_iq, block_size, block_size);                        // asynchronous on the stream given
//   mon.Update();                                                      // waits, reads 1.8 KB + 1.2 KB per station
//   mon.DeviationHz(c); mon.OffsetHz(c); mon.PilotHz(c); mon.MpxPowerDbr(c, 60); mon.Exceedance(c, 75000);
#pragma once

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class ModulationMonitor_GPU {
    fmd_modmon m = nullptr;
    int n_channels;
    fmd_modmon_design_t design{};
    std::vector<fmd_modmon_status> status;
    std::vector<unsigned> hist;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_modmon_last_error(m)); }
    static double nan() { return std::numeric_limits<double>::quiet_NaN(); }
public:
    ModulationMonitor_GPU(int _n_channels, int fs, long long max_input_samples, int device = -1)
        : n_channels(_n_channels), status((size_t)(_n_channels > 0 ? _n_channels : 0)), hist((size_t)(_n_channels > 0 ? _n_channels : 0) * 300) {
        fmd_modmon_config cfg{_n_channels, fs, max_input_samples, device};
        if (fmd_modmon_create(&cfg, &m) != FMD_OK) throw std::runtime_error(std::string("fmd_modmon_create: ") + fmd_modmon_last_error(nullptr));
        fmd_modmon_design(fs, &design);
    }
    ~ModulationMonitor_GPU() { if (m) fmd_modmon_destroy(m); }
    ModulationMonitor_GPU(const ModulationMonitor_GPU&) = delete;
    ModulationMonitor_GPU& operator=(const ModulationMonitor_GPU&) = delete;

    int GetTotalChannels() const { return n_channels; }
    const fmd_modmon_design_t& Design() const { return design; }

    // monitors n samples of every station whose d_active byte is not 0 (NULL: all); asynchronous on `stream`
    void Process(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        check(fmd_modmon_process_cf32_dev(m, d_in, in_stride, n, d_active, stream), "fmd_modmon_process_cf32_dev");
    }
    void Process(const uint8_t* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        check(fmd_modmon_process_u8_dev(m, d_in, in_stride, n, d_active, stream), "fmd_modmon_process_u8_dev");
    }
    void Reset(int channel = -1) { check(fmd_modmon_reset(m, channel), "fmd_modmon_reset"); }
    void ResetPeaks(int channel = -1) { check(fmd_modmon_reset_peaks(m, channel), "fmd_modmon_reset_peaks"); }

    // waits for the monitor's work and copies every station's record and histogram to the host
    void Update() {
        check(fmd_modmon_get_status(m, status.data()), "fmd_modmon_get_status");
        check(fmd_modmon_get_histogram(m, hist.data()), "fmd_modmon_get_histogram");
    }
    // as of the last Update()
    const fmd_modmon_status& Status(int c) const { return status.at((size_t)c); }
    const unsigned* Histogram(int c) const { return &hist.at((size_t)c * 300); }
    // Hz, of the newest 50 ms interval; NaN before the first
    double DeviationHz(int c) const { double v = 0.0; return fmd_modmon_deviation_hz(&Status(c), &design, &v) == FMD_OK ? v : nan(); }
    double OffsetHz(int c) const { double v = 0.0; return fmd_modmon_offset_hz(&Status(c), &design, &v) == FMD_OK ? v : nan(); }
    double PilotHz(int c) const { double v = 0.0; return fmd_modmon_pilot_hz(&Status(c), &design, &v) == FMD_OK ? v : nan(); }
    // dBr over the newest window_s completed seconds; NaN while fewer are complete
    double MpxPowerDbr(int c, int window_s = 60) const {
        double v = 0.0;
        return fmd_modmon_mpx_power_dbr(&Status(c), &design, window_s, &v) == FMD_OK ? v : nan();
    }
    // the fraction of intervals since reset whose peak deviation is at least limit_hz; NaN before the first
    double Exceedance(int c, int limit_hz = 75000, unsigned long long* count = nullptr) const {
        double f = 0.0;
        unsigned long long n = 0;
        if (fmd_modmon_exceedance(Histogram(c), Status(c).over, limit_hz, &f, &n) != FMD_OK) return nan();
        if (count) *count = n;
        return f;
    }
    double PercentileHz(int c, double q) const { double v = 0.0; return fmd_modmon_percentile(Histogram(c), Status(c).over, q, &v) == FMD_OK ? v : nan(); }
    // the device's own records, for a consumer on the device (valid until the next Process)
    const fmd_modmon_status* StatusDev() const {
        const fmd_modmon_status* p = nullptr;
        check(fmd_modmon_status_dev(m, &p), "fmd_modmon_status_dev");
        return p;
    }
};

}  // namespace fmd_host
