// Host-side half of the log-mel front end (fmd_logmel.hip): the configuration's validation, the window, the cos / sin table, the mel
// filterbank and the launch layout the kernel shares with the host (include/fmdemod.h, "Log-mel front end"), in double.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kLogmelTile = 16;                 // rows (spectral frames) and columns (bins, bands) of an MFMA tile
constexpr int kLogmelLdsBytes = 64 * 1024;      // what a workgroup's LDS image may take

// where a workgroup's LDS image lies (float offsets) for a valid configuration, and the padded sizes
struct LogmelLayout {
    int K, Kp;            // bins, and bins padded to a multiple of 16
    int Mp;               // bands padded to a multiple of 16
    int rows;             // spectral frames a pass takes: the most, up to 16, whose samples and powers fit the LDS image
    int span;             // mono samples of a pass: (rows - 1) hop + N
    int off_w, off_tab, off_m, off_p, off_nf, total;   // w [N], (cos, sin) [N][2], m [span], P [rows][Kp], nonfinite flags [16]; floats in all
};

// the message of the last failing call that has no handle (fmd_logmel_create and the host-only functions)
std::string& logmel_global_error();
// FMD_OK for a valid configuration; FMD_ERR_ARG and the reason in *err otherwise
int logmel_check(const fmd_logmel_config* cfg, std::string* err);
// K of a checked configuration
int logmel_bins(const fmd_logmel_config* cfg);
// T(f): spectral frames complete after f audio frames (constexpr: the kernel calls it too)
constexpr unsigned long long logmel_spectra(unsigned long long f, int win, int hop) {
    return f < (unsigned long long)win ? 0ull : (f - (unsigned long long)win) / (unsigned long long)hop + 1ull;
}
// the LDS layout of a checked configuration
LogmelLayout logmel_layout(const fmd_logmel_config* cfg);

}  // namespace fmd
