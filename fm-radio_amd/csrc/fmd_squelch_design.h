// Host-side half of the carrier squelch (fmd_squelch.hip): the parameters' validation and derived figures, the read-out functions and the
// layout constants the kernel shares with them (include/fmdemod.h, "Carrier squelch"), in double.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kSquelchPartials = 256;   // NP: partial sums per interval sum (four per lane)
constexpr int kSquelchRing = 20;        // intervals kept per station (one second)

// what the kernel reads of a station's parameters
struct SquelchGate {
    double c_open, c_close, min_s2;
    int open_intervals, close_intervals, mode, reserved;
};

// the message of the last failing call that has no squelch handle (fmd_squelch_create, the read-out functions)
std::string& squelch_global_error();
// M = fs / 20, or 0 unless fs is a multiple of 1000 in 192000 ... 384000
int squelch_interval(int fs);
// FMD_OK and *out for valid parameters; FMD_ERR_ARG and the reason in *err otherwise
int squelch_gate(const fmd_squelch_params* p, int M, SquelchGate* out, std::string* err);

}  // namespace fmd
