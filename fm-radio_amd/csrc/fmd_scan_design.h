// Host-side half of the band scanner (fmd_scan.hip): the default FFT size, the default detection parameters and the detection rules
// (include/fmdemod.h, "Band scan"), a pure function of the PSD in double.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

// nfft a power of two in [256, 16384]
bool scan_nfft_ok(int nfft);
// the message of the last failing call that has no scanner handle (fmd_scan_detect, fmd_scan_create)
std::string& scan_global_error();
// fmd_scan_detect; on FMD_ERR_ARG *err holds the reason
int scan_detect(const double* psd, int nfft, double fs_in, const fmd_scan_params* p, fmd_scan_station* out, int cap, int* n_found,
                std::string* err);

}  // namespace fmd
