// Host-side half of the FLAC audio encoder (fmd_flac.hip): the block geometry, the frame size bound, the calls' parameter checks, the
// CRC tables the kernels read, the stream header and the matching decoder (include/fmdemod.h, "FLAC audio encoder").  All integer.
// Needs no GPU.
#pragma once
#include <cstdint>
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kFlacDefaultBlock = 4096;      // frames of a block where the configuration says 0
constexpr int kFlacMaxBlock = 4608;          // the streamable subset's largest block at 48 kHz and below
constexpr int kFlacStreamHeader = 42;        // `fLaC`, a metadata block header and STREAMINFO's 34 bytes
constexpr unsigned kFlacCrc16Poly = 0x8005u;

// the message of the last failing call that has no encoder handle (fmd_flac_create, the host-only functions)
std::string& flac_global_error();
// S itself (kFlacDefaultBlock for 0), or 0 unless S is a multiple of 64 in 64 ... 4608
int flac_block_frames(int S);
// the most bytes of a frame of up to S frames: 16 of header, two VERBATIM subframes (the 17-bit side channel counted for both), CRC-16
constexpr int flac_frame_bound(int S) { return 16 + 2 * (1 + 2 * S) + 2; }
// the most bytes a process call of n frames writes for a station, whatever its fill, rounded up to 4
constexpr long long flac_max_bytes(int S, long long n) { return (((long long)(S - 1) + n) / S * flac_frame_bound(S) + 3) / 4 * 4; }
// FMD_OK for a process call the encoder takes; FMD_ERR_ARG and the reason in *err otherwise
int flac_check_call(int S, long long max_in, const void* d_in, long long in_stride, long long n, const void* d_out, long long out_stride, std::string* err);
// what the kernels read: crc16[256], the CRC-16 of each single byte, then pow[m] = x^(8 m) mod P for m = 0 ... n_pow - 1
// (the CRC is linear: crc(A | B) = crc(A) * x^(8 |B|) + crc(B)); `out` holds 256 + n_pow entries
void flac_crc16_tables(int n_pow, uint16_t* out);
unsigned flac_crc8(const uint8_t* p, long long n);
unsigned flac_crc16(const uint8_t* p, long long n);

}  // namespace fmd
