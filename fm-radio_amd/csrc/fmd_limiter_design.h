// Host-side half of the look-ahead peak limiter (fmd_limiter.hip): the design (D, step, T from milliseconds and decibels), the
// default configuration, the loudness helper and the process call's parameter checks (include/fmdemod.h, "Look-ahead peak limiter").
// Double and host libm; the kernels take W, step and T as numbers.  Needs no GPU.
#pragma once
#include <cstdint>
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr uint32_t kLimiterOne = 1u << 30;   // ONE: unity gain in Q30
constexpr int kLimiterMaxD = 255;            // the longest look-ahead, in frames

// the message of the last failing call that has no limiter handle (fmd_limiter_create, the host-only functions)
std::string& limiter_global_error();
// FMD_OK for a process call the limiter takes; FMD_ERR_ARG and the reason in *err otherwise
int limiter_check_call(int C, long long max_in, const void* d_in, long long in_stride, long long n, const void* d_out, long long out_stride, std::string* err);

}  // namespace fmd
