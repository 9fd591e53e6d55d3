// Host-side half of the FM modulation monitor (fmd_modmon.hip): the design, the read-out functions and the layout constants the kernel
// shares with them (include/fmdemod.h, "FM modulation monitor"), in double.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kModmonTaps = 33;      // T: taps of the MPX low-pass
constexpr int kModmonHist = kModmonTaps - 1;   // values of d the filter needs behind a sample
constexpr int kModmonPartials = 64;  // NP: partial sums per interval sum (one per lane)
constexpr int kModmonBins = 300;     // NB: histogram bins of 500 Hz from 0
constexpr int kModmonRing = 60;      // seconds kept per station
constexpr int kModmonMaxP = 384;     // longest pilot table
constexpr int kModmonIntervalsPerSecond = 20;
constexpr double kModmonBinHz = 500.0;

// the message of the last failing call that has no monitor handle (fmd_modmon_design, fmd_modmon_create, the read-out functions)
std::string& modmon_global_error();
// fmd_modmon_design; on FMD_ERR_ARG *err holds the reason
int modmon_design(int fs, fmd_modmon_design_t* out, std::string* err);

}  // namespace fmd
