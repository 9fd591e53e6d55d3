// Host-side half of the loudness meter (fmd_meter.hip): the filter and histogram design and the read-out functions
// (include/fmdemod.h, "Batched loudness meter"), in double.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kMeterBins = 1000;     // histogram bins of 0.1 LU from -70 LUFS
constexpr int kMeterRing = 30;       // sub-block energies kept per station (3 s: the short-term window)
constexpr int kMeterTpTaps = 12;     // taps per phase of the true-peak interpolator
constexpr int kMeterTpHist = kMeterTpTaps - 1;   // frames of history it carries per (station, rail)

// the message of the last failing call that has no meter handle (fmd_meter_design, fmd_meter_create, the read-out functions)
std::string& meter_global_error();
// fmd_meter_design; on FMD_ERR_ARG *err holds the reason
int meter_design(int fs, fmd_meter_design_t* out, std::string* err);
// fmd_meter_tp_design, likewise
int meter_tp_design(int fs, fmd_meter_tp_design_t* out, std::string* err);

}  // namespace fmd
