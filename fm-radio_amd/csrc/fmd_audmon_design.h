// Host-side half of the audio fault monitor (fmd_audmon.hip): the parameters' validation and derived thresholds, the read-out functions
// and the layout constants the kernel shares with them (include/fmdemod.h, "Audio fault monitor"), in double.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kAudmonPartials = 64;     // NP: partial sums per interval sum (one per lane)
constexpr int kAudmonRing = 30;         // intervals kept per station (three seconds)
constexpr int kAudmonDetectors = 5;

// what the kernel reads of a station's parameters
struct AudmonGate {
    double min_e, c_loss, c_anti, c_mono;
    int raise_intervals[kAudmonDetectors], clear_intervals[kAudmonDetectors];
    unsigned alarm_mask;
    int reserved;
};

// the message of the last failing call that has no monitor handle (fmd_audmon_create, the read-out functions)
std::string& audmon_global_error();
// M = fs / 10, or 0 unless fs is a multiple of 10 in 8000 ... 192000
int audmon_interval(int fs);
// FMD_OK and *out for valid parameters; FMD_ERR_ARG and the reason in *err otherwise
int audmon_gate(const fmd_audmon_params* p, int M, AudmonGate* out, std::string* err);

}  // namespace fmd
