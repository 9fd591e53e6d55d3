// Host-side half of the audio fingerprinter (fmd_fprint.hip): the configuration's validation, the band edges, the sub-block basis, the
// frame twiddles and the sizes the kernels share with the host (include/fmdemod.h, "Audio fingerprinter"), in double.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kFprintTile = 16;                 // rows and columns of an MFMA tile
constexpr int kFprintMaxBands = 33;
constexpr int kFprintChunk = 64;                // bins of a chunk of k_fprint_frame (two more are read, one on each side)
constexpr int kFprintMaxPiece = 32;             // the most sub-blocks of a station a piece of a call completes
constexpr int kFprintScratchBytes = 64 * 1024;  // what a station's rows of the per-call scratch may take

// the sizes of a checked, valid design
struct FprintLayout {
    int N;                // R H
    int K, Kp;            // transformed bins, and bins padded to a multiple of 16; a spectrum row is [2][Kp]: re, then im
    int first_bin;        // k_0 - 1
    int piece;            // sub-blocks of a station a piece completes at most: 1 ... 32, no more than a call of max_input_frames gives
                          // and no more than fit kFprintScratchBytes (but at least 2)
    long long piece_frames;   // frames of a piece: piece * H
    int lds_floats;       // k_fprint_frame's LDS image
    int edges[kFprintMaxBands + 1];   // k_b
};

// the message of the last failing call that has no handle (fmd_fprint_create and the host-only functions)
std::string& fprint_global_error();
// FMD_OK for a valid configuration (ranges only); FMD_ERR_ARG and the reason in *err otherwise
int fprint_check(const fmd_fprint_config* cfg, std::string* err);
// the edges and sizes of a range-checked configuration; FMD_ERR_ARG and the reason where the design is invalid
int fprint_layout(const fmd_fprint_config* cfg, FprintLayout* out, std::string* err);
// device bytes of `channels` stations of a valid design
long long fprint_bytes(const fmd_fprint_config* cfg, const FprintLayout& L, long long channels);

}  // namespace fmd
