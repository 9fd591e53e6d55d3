// Header-only C++ host adaptor over the C ABI's batched loudness meter (include/fmdemod.h "Batched loudness meter"): RAII around the
// handle, exceptions instead of status codes, and the read-out in LUFS.  NOT in the reference (williamyang98/FM-Radio has no meter): it
// sits beside the resampler and the mixer and reads the same device audio array [C][in_stride][2], e.g. fmd_audio_dev's view:
//
//   fmd_host::LoudnessMeter_GPU meter(n_channels, rates.fs_audio, rates.n_audio);
//   meter.Process(d_audio, rates.n_audio, rates.n_audio);            // asynchronous on the stream given
//   meter.Update();                                                   // waits, reads the few hundred bytes per station
//   meter.Integrated(c); meter.Momentary(c); meter.Status(c).peak_hold[0];
//
// With features (FMD_METER_TRUE_PEAK | FMD_METER_RANGE as the constructor's last argument) Update() also reads the 24-byte r128 records
// and the range histograms: meter.TruePeakDbtp(c, rail); meter.LoudnessRange(c);
#pragma once

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class LoudnessMeter_GPU {
    fmd_meter m = nullptr;
    int n_channels;
    fmd_meter_design_t design{};
    std::vector<fmd_meter_status> status;
    std::vector<unsigned> hist;
    unsigned features;
    std::vector<fmd_meter_r128_status> r128;
    std::vector<unsigned> range_hist;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_meter_last_error(m)); }
public:
    LoudnessMeter_GPU(int _n_channels, int fs, long long max_input_frames, int device = -1, unsigned _features = 0)
        : n_channels(_n_channels), status((size_t)(_n_channels > 0 ? _n_channels : 0)), hist((size_t)(_n_channels > 0 ? _n_channels : 0) * 1000),
          features(_features), r128(_features ? status.size() : 0), range_hist((_features & FMD_METER_RANGE) ? hist.size() : 0) {
        fmd_meter_config cfg{_n_channels, fs, max_input_frames, device};
        if (fmd_meter_create_ex(&cfg, features, &m) != FMD_OK) throw std::runtime_error(std::string("fmd_meter_create_ex: ") + fmd_meter_last_error(nullptr));
        fmd_meter_design(fs, &design);
    }
    ~LoudnessMeter_GPU() { if (m) fmd_meter_destroy(m); }
    LoudnessMeter_GPU(const LoudnessMeter_GPU&) = delete;
    LoudnessMeter_GPU& operator=(const LoudnessMeter_GPU&) = delete;

    int GetTotalChannels() const { return n_channels; }
    const fmd_meter_design_t& Design() const { return design; }
    unsigned Features() const { return features; }

    // meters n frames of every station whose d_active byte is not 0 (NULL: all); asynchronous on `stream`
    void Process(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        check(fmd_meter_process_f32_dev(m, d_in, in_stride, n, d_active, stream), "fmd_meter_process_f32_dev");
    }
    void Reset(int channel = -1) { check(fmd_meter_reset(m, channel), "fmd_meter_reset"); }
    void ResetPeaks(int channel = -1) { check(fmd_meter_reset_peaks(m, channel), "fmd_meter_reset_peaks"); }

    // waits for the meter's work and copies every station's record and histogram to the host
    void Update() {
        check(fmd_meter_get_status(m, status.data()), "fmd_meter_get_status");
        check(fmd_meter_get_histogram(m, hist.data()), "fmd_meter_get_histogram");
        if (features) check(fmd_meter_get_r128_status(m, r128.data()), "fmd_meter_get_r128_status");
        if (features & FMD_METER_RANGE) check(fmd_meter_get_range_histogram(m, range_hist.data()), "fmd_meter_get_range_histogram");
    }
    // as of the last Update()
    const fmd_meter_status& Status(int c) const { return status.at((size_t)c); }
    const unsigned* Histogram(int c) const { return hist.data() + (size_t)c * 1000; }
    // LUFS; -inf where nothing passed the -70 LUFS gate, NaN while the window is not full yet
    double Integrated(int c) const {
        double v = 0.0;
        check(fmd_meter_integrated(Histogram(c), &design, &v), "fmd_meter_integrated");
        return v;
    }
    double Momentary(int c) const {
        double v = 0.0;
        return fmd_meter_momentary(&Status(c), &v) == FMD_OK ? v : std::numeric_limits<double>::quiet_NaN();
    }
    double ShortTerm(int c) const {
        double v = 0.0;
        return fmd_meter_short_term(&Status(c), &v) == FMD_OK ? v : std::numeric_limits<double>::quiet_NaN();
    }
    // with a feature, as of the last Update(); std::out_of_range on a meter without it
    const fmd_meter_r128_status& R128(int c) const { return r128.at((size_t)c); }
    const unsigned* RangeHistogram(int c) const { return &range_hist.at((size_t)c * 1000); }
    // the held maximum true-peak level of a rail in dBTP; -inf for silence
    double TruePeakDbtp(int c, int rail) const { return fmd_meter_dbtp(R128(c).tp_hold[rail & 1]); }
    // LU; low / high (may be NULL): the 10th / 95th percentile in LUFS.  NaN while no short-term value passes the gates
    double LoudnessRange(int c, double* low = nullptr, double* high = nullptr) const {
        double lra = 0.0, lo = 0.0, hi = 0.0;
        if (fmd_meter_range(RangeHistogram(c), &design, &lra, &lo, &hi) != FMD_OK) lra = lo = hi = std::numeric_limits<double>::quiet_NaN();
        if (low) *low = lo;
        if (high) *high = hi;
        return lra;
    }
    // the device's own records, for a consumer on the device (valid until the next Process)
    const fmd_meter_r128_status* R128Dev() const {
        const fmd_meter_r128_status* p = nullptr;
        check(fmd_meter_r128_status_dev(m, &p), "fmd_meter_r128_status_dev");
        return p;
    }
    const fmd_meter_status* StatusDev() const {
        const fmd_meter_status* p = nullptr;
        check(fmd_meter_status_dev(m, &p), "fmd_meter_status_dev");
        return p;
    }
};

}  // namespace fmd_host
