// The sample formats of a wideband capture, shared by the channeliser (fmd_channelizer.hip) and the band scanner (fmd_scan.hip): cf32,
// or a receiver's interleaved integers — u8 (RTL-SDR), s8 (HackRF), s16 (Airspy, SDRplay, USRP sc16).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fmd {

// One I / Q pair of the caller's block: `raw`, what one load fetches (all of the pair), and cf32(), its exact conversion.  A conversion
// is a separate rounding-free step: every integer of these types is a float, and v - 127 of a u8 is exact (-ffp-contract=off keeps it
// out of the mixer's fmaf).  zero() is the raw pair that converts to (+0, +0): what a window sample outside the data reads as.
template <typename S> struct Iq;
template <> struct Iq<float2> {
    using raw = float2;
    static __device__ __forceinline__ raw zero() { return make_float2(0.f, 0.f); }
    static __device__ __forceinline__ const float2& cf32(const raw& v) { return v; }   // (no copy: the cf32 kernels' code stays as it was)
};
template <> struct Iq<uint8_t> {          // RTL-SDR: the reference's (float)u8 - 127 (src/app.cpp), as fmd_process_u8_* takes it
    using raw = unsigned short;
    static __device__ __forceinline__ raw zero() { return 0x7f7f; }
    static __device__ __forceinline__ float2 cf32(raw v) { return make_float2((float)(v & 0xffu) - 127.0f, (float)(v >> 8) - 127.0f); }
};
template <> struct Iq<int8_t> {           // HackRF
    using raw = unsigned short;
    static __device__ __forceinline__ raw zero() { return 0; }
    static __device__ __forceinline__ float2 cf32(raw v) { return make_float2((float)(signed char)(v & 0xffu), (float)(signed char)(v >> 8)); }
};
template <> struct Iq<int16_t> {          // Airspy, SDRplay, USRP sc16
    using raw = unsigned int;
    static __device__ __forceinline__ raw zero() { return 0; }
    static __device__ __forceinline__ float2 cf32(raw v) { return make_float2((float)(short)(v & 0xffffu), (float)(short)(v >> 16)); }
};

}  // namespace fmd
