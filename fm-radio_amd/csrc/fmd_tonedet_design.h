// Host-side half of the audio tone detector (fmd_tonedet.hip): the cos / sin table, the parameters' validation and derived thresholds,
// the read-out functions and the layout constants the kernel shares with them (include/fmdemod.h, "Audio tone detector"), in double.
// Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kTonedetPartials = 64;    // NP: partial sums per interval sum (one per lane)
constexpr int kTonedetRing = 30;        // intervals kept per station (three seconds)
constexpr int kTonedetSlots = 8;        // NS: tone slots per station
constexpr int kTonedetSums = 1 + 2 * kTonedetSlots;   // mm, then re and im of slot 0, 1, ...

// what the kernel reads of a station's parameters; freq_hz is pending until an interval starts
struct TonedetGate {
    double min_e, c[kTonedetSlots];
    int freq_hz[kTonedetSlots], raise_intervals[kTonedetSlots], clear_intervals[kTonedetSlots];
    unsigned alarm_mask;
    int reserved;
};

// the message of the last failing call that has no detector handle (fmd_tonedet_create, the read-out functions)
std::string& tonedet_global_error();
// M = fs / 10, or 0 unless fs is a multiple of 10 in 8000 ... 48000
int tonedet_interval(int fs);
// FMD_OK and *out for valid parameters; FMD_ERR_ARG and the reason in *err otherwise
int tonedet_gate(const fmd_tonedet_params* p, int fs, TonedetGate* out, std::string* err);
// tab [fs][2]: cos and sin of 2 pi j / fs
void tonedet_table(int fs, double* tab);

}  // namespace fmd
