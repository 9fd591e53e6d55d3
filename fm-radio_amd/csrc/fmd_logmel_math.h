// Device math of the log-mel front end (fmd_logmel.hip): flog10, a base-10 logarithm as a fixed sequence of IEEE operations.
//
// The log-mel object's rows are compared bit for bit with tests/cpp/logmel_ref.c, so its logarithm cannot be a libm's, device or host:
// those may change with the toolchain.  flog10 is spelled here (and in include/fmdemod.h, "Log-mel front end") with integer operations,
// +, *, fmaf and selects only; the translation units that include this header are built with -ffp-contract=off, so every operation is
// the one written and rounds once.  The header also compiles as plain host C++ (FMDL_HD static inline): the host-only exhaustive sweep
// (tools/logmel_flog10_sweep.cpp) and the library's fmd_logmel_flog10 evaluate the very same lines.
//
//   x = 2^e (1 + f),  1 + f in [sqrt(1/2), sqrt(2)):   u = bits(x) - 0x3f3504f3;  e = (int)u >> 23;  1 + f = bits((u & 0x7fffff) + 0x3f3504f3)
//   R(f) = c1 + f (c2 + ... + f c11)                   Horner in fmaf; the degree-11 Chebyshev interpolant of log10(1 + f) / f on the
//                                                      interval, less its constant term 1 / ln 10 = C0hi + C0lo
//   lm   = fmaf(f, C0hi, f * fmaf(f, R, C0lo))         log10(1 + f); relative, not absolute, accuracy near x = 1
//   y    = fmaf(e, L2hi, fmaf(e, L2lo, lm))            L2hi = log10(2) cut to 11 bits: e * L2hi is exact
//   +inf -> +inf, NaN -> NaN (the argument itself).  The argument is never below FLT_MIN (the caller's floor): denormals, zero and
//   negative numbers are not in its domain.
// Worst case over every finite float >= FLT_MIN against float64 log10: DESIGN.md §6n.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FMDL_HD __host__ __device__ __forceinline__
#else
#define FMDL_HD static inline
#endif

namespace fmd {

FMDL_HD float lm_bits_f32(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f; memcpy(&f, &u, 4); return f;
#endif
}
FMDL_HD uint32_t lm_f32_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u; memcpy(&u, &f, 4); return u;
#endif
}

constexpr uint32_t kFlogSqrtHalf = 0x3f3504f3u;   // (float)sqrt(1/2)
constexpr uint32_t kFlogC0hi = 0x3ede5bd9u;       // (float)(1 / ln 10)
constexpr uint32_t kFlogC0lo = 0xb22d91afu;       // (float)(1 / ln 10 - C0hi)
constexpr uint32_t kFlogL2hi = 0x3e9a2000u;       // log10(2) cut to 11 bits
constexpr uint32_t kFlogL2lo = 0x369a84fcu;       // (float)(log10(2) - L2hi)
constexpr uint32_t kFlogC[11] = {0xbe5e5bd9u, 0x3e143d3au, 0xbdde5bb4u, 0x3db1e377u, 0xbd9445b2u, 0x3d7e1719u,
                                 0xbd5cc607u, 0x3d446f9au, 0xbd41dcffu, 0x3d3d35d2u, 0xbccff948u};   // c1 ... c11

FMDL_HD float flog10(float x) {
    const uint32_t ix = lm_f32_bits(x);
    const uint32_t u = ix - kFlogSqrtHalf;
    const float ef = (float)((int32_t)u >> 23);
    const float f = lm_bits_f32((u & 0x007fffffu) + kFlogSqrtHalf) - 1.0f;             // exact: 1 + f lies in [1/2, 2]
    float r = lm_bits_f32(kFlogC[10]);
    r = fmaf(f, r, lm_bits_f32(kFlogC[9]));
    r = fmaf(f, r, lm_bits_f32(kFlogC[8]));
    r = fmaf(f, r, lm_bits_f32(kFlogC[7]));
    r = fmaf(f, r, lm_bits_f32(kFlogC[6]));
    r = fmaf(f, r, lm_bits_f32(kFlogC[5]));
    r = fmaf(f, r, lm_bits_f32(kFlogC[4]));
    r = fmaf(f, r, lm_bits_f32(kFlogC[3]));
    r = fmaf(f, r, lm_bits_f32(kFlogC[2]));
    r = fmaf(f, r, lm_bits_f32(kFlogC[1]));
    r = fmaf(f, r, lm_bits_f32(kFlogC[0]));
    const float t = fmaf(f, r, lm_bits_f32(kFlogC0lo));
    const float lm = fmaf(f, lm_bits_f32(kFlogC0hi), f * t);
    const float y = fmaf(ef, lm_bits_f32(kFlogL2hi), fmaf(ef, lm_bits_f32(kFlogL2lo), lm));
    return (ix & 0x7fffffffu) >= 0x7f800000u ? x : y;                                   // +inf and NaN: the argument
}

// what mode 1 takes the logarithm of: the band above the floor, the floor, or the band's NaN
FMDL_HD float logmel_clamp(float mel, float floor) { return mel > floor ? mel : (mel != mel ? mel : floor); }

// a band as written: mode 0 the band, mode 1 flog10 of the clamped band; any NaN leaves as the quiet NaN 0x7fc00000, whatever payload
// or sign the chains gave it (those differ between processors, and rows compare bit for bit)
FMDL_HD float logmel_out(float mel, int out_mode, float floor) {
    const float v = out_mode ? flog10(logmel_clamp(mel, floor)) : mel;
    return v != v ? lm_bits_f32(0x7fc00000u) : v;
}

}  // namespace fmd
