// Host-side half of the ADPCM audio encoder (fmd_adpcm.hip): the IMA / DVI tables, the block geometry, the process call's parameter
// checks, the matching decoder and the WAV header (include/fmdemod.h, "ADPCM audio encoder").  All integer.  Needs no GPU.
#pragma once
#include <cstdint>
#include <string>

#include "fmdemod.h"

// the published IMA / DVI step sizes, index 0 ... 88 (one list for the host table and the kernels' constant array)
#define FMD_ADPCM_STEP_TABLE                                                                                                                 \
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157,   \
    173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707,      \
    1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635,        \
    13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767

namespace fmd {

constexpr int kAdpcmSteps = 89;              // entries of the step table
constexpr int kAdpcmDefaultBlock = 1017;     // frames of a block where the configuration says 0: 1024 bytes
constexpr int kAdpcmMaxBlock = 8185;         // the largest block: 8192 bytes
constexpr int kAdpcmWavHeader = 60;          // bytes of the RIFF header: RIFF 12, fmt 8 + 20, fact 8 + 4, data 8

extern const int kAdpcmStep[kAdpcmSteps];
extern const int kAdpcmIndexAdjust[8];       // by the code's three magnitude bits

// the message of the last failing call that has no encoder handle (fmd_adpcm_create, the host-only functions)
std::string& adpcm_global_error();
// S itself (kAdpcmDefaultBlock for 0), or 0 unless S = 1 (mod 8) in 9 ... 8185
int adpcm_block_frames(int S);
// bytes of a block of S frames (S valid): 8 of header and 8 per further eight frames
constexpr int adpcm_block_align(int S) { return 8 * ((S - 1) / 8 + 1); }
// FMD_OK for a process call the encoder takes; FMD_ERR_ARG and the reason in *err otherwise
int adpcm_check_call(int S, long long max_in, const void* d_in, long long in_stride, long long n, const void* d_out, long long out_stride, std::string* err);

}  // namespace fmd
