// Host-side half of the IQ corrector (fmd_iqcorr.hip): the solve step and the halving tree of a chunk's 256 partial sums
// (include/fmdemod.h, "DC offset and IQ imbalance correction"), in double.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kIqChunk = 4096;     // samples per chunk of the moments' summation order
constexpr int kIqLanes = 256;      // partial sums per chunk and moment
constexpr int kIqMoments = 5;      // sum i, sum q, sum i^2, sum q^2, sum i q (n is a count)

// the message of the last failing call that has no corrector handle (fmd_iqcorr_solve, fmd_iqcorr_create)
std::string& iqcorr_global_error();
// p_j += p_{j + 128} for j < 128, then 64, ... 1, in place; returns p_0
double iqcorr_tree(double* p);
// fmd_iqcorr_solve; on FMD_ERR_ARG *err holds the reason
int iqcorr_solve(const fmd_iq_moments* m, fmd_iq_correction* out, std::string* err);
bool iqcorr_finite(const fmd_iq_correction& c);

}  // namespace fmd
