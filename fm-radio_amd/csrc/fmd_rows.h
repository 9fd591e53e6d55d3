// The row walk of the interval monitors (k_squelch, k_audmon, k_tonedet), stated once, and the small pieces that k_modmon shares with
// them.  Device code; included by fmd_squelch.hip, fmd_audmon.hip, fmd_tonedet.hip and fmd_modmon.hip only.
//
// Geometry: one wavefront of 64 lanes per station over rows of 256 consecutive samples (IQ pairs or audio frames) that start at a
// multiple of 256 of r, r the sample's place in its interval of M samples.  Lane l loads samples 4 l ... 4 l + 3 of a row at once
// (non-temporal: the input is read once), kPf rows in registers ahead of the rows at hand.  A call is walked in segments that end with
// their interval or with the call, so the first row of a call and the rows around an interval's end are partial: a lane's sample
// outside the segment at hand is not loaded and reads as `zero`, the raw sample that converts to (+0, +0) and so changes no partial of a
// sum and no peak.  An interval's end is wave-uniform.
#pragma once
#include <hip/hip_runtime.h>

namespace fmd {
namespace rows {

constexpr int kT = 64;               // lanes: one wavefront, one station
constexpr int kQ = 4;                // samples per lane and row
constexpr int kRow = kT * kQ;        // samples per row

// A lane's four samples of a row, loaded at once, and one sample alone.  The station's rows are aligned to a sample only (8 bytes of
// cf32 or of an L, R frame, 2 of u8): the types carry that alignment, and the device's global loads take any.
typedef float f4 __attribute__((ext_vector_type(4), aligned(8)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned u2 __attribute__((ext_vector_type(2), aligned(2)));

__device__ __forceinline__ void load4(const float2* p, float2 (&z)[kQ]) {
    const f4 a = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
    const f4 b = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p + 2));
    z[0] = make_float2(a.x, a.y); z[1] = make_float2(a.z, a.w); z[2] = make_float2(b.x, b.y); z[3] = make_float2(b.z, b.w);
}
__device__ __forceinline__ void load4(const unsigned short* p, unsigned short (&z)[kQ]) {
    const u2 a = __builtin_nontemporal_load(reinterpret_cast<const u2*>(p));
    z[0] = (unsigned short)(a.x & 0xffffu); z[1] = (unsigned short)(a.x >> 16); z[2] = (unsigned short)(a.y & 0xffffu); z[3] = (unsigned short)(a.y >> 16);
}
__device__ __forceinline__ float2 load1(const float2* p) {
    const f2 v = __builtin_nontemporal_load(reinterpret_cast<const f2*>(p));
    return make_float2(v.x, v.y);
}
__device__ __forceinline__ unsigned short load1(const unsigned short* p) { return __builtin_nontemporal_load(p); }

// The lane's samples of the kPf rows from `row` on: four at once where all four are in the segment [s0, seg_end), one by one where the
// segment's edge runs through them, `zero` outside.
template <int kPf, typename Raw>
__device__ __forceinline__ void fetch_rows(const Raw* base, int lane, long long row, long long s0, long long seg_end, Raw zero, Raw (&nxt)[kPf][kQ]) {
#pragma unroll
    for (int p = 0; p < kPf; p++) {
        const long long i = row + (long long)p * kRow + kQ * lane;
        if (i >= s0 && i + kQ <= seg_end) load4(base + i, nxt[p]);
        else {
#pragma unroll
            for (int k = 0; k < kQ; k++) {
                nxt[p][k] = zero;
                if (i + k >= s0 && i + k < seg_end) nxt[p][k] = load1(base + i + k);
            }
        }
    }
}

// The walk over the n samples at `base` of a station whose first sample is at place r0 of its interval.  Per segment:
//   start(r0)        at its start, r0 its first sample's place;
//   body(v)          per row in ascending order, v the lane's four raw samples of it;
//   tail(complete)   at its end, `complete` when the interval ends with it (wave-uniform).
// The hooks' accumulators are the caller's locals, captured by reference.  r0 is taken by value: the walk advances its own copy, and
// the caller's is not changed (the place of the next call's first sample follows from the record's counters).
template <int kPf, typename Raw, typename Start, typename Body, typename Tail>
__device__ __forceinline__ void walk(const Raw* base, int lane, long long n, int M, int r0, Raw zero, Start&& start, Body&& body, Tail&& tail) {
    long long s0 = 0;                                                        // the segment's first sample
    while (s0 < n) {
        const long long left = (long long)(M - r0);
        const long long seg_end = n - s0 < left ? n : s0 + left;
        const long long rb = s0 - (long long)(r0 & (kRow - 1));              // the first row's sample 0 (before s0: those samples read as zero)
        start(r0);

        Raw nxt[kPf][kQ];
        fetch_rows<kPf>(base, lane, rb, s0, seg_end, zero, nxt);
        for (long long row = rb; row < seg_end; row += (long long)kPf * kRow) {
            Raw cur[kPf][kQ];
#pragma unroll
            for (int p = 0; p < kPf; p++)
#pragma unroll
                for (int k = 0; k < kQ; k++) cur[p][k] = nxt[p][k];
            if (row + (long long)kPf * kRow < seg_end) fetch_rows<kPf>(base, lane, row + (long long)kPf * kRow, s0, seg_end, zero, nxt);   // in flight while these rows run
#pragma unroll
            for (int p = 0; p < kPf; p++)
                if (row + (long long)p * kRow < seg_end) body(cur[p]);
        }

        r0 += (int)(seg_end - s0);
        const bool complete = r0 == M;
        tail(complete);
        if (complete) r0 = 0;
        s0 = seg_end;
    }
}
template <int kPf, typename Raw, typename Body, typename Tail>
__device__ __forceinline__ void walk(const Raw* base, int lane, long long n, int M, int r0, Raw zero, Body&& body, Tail&& tail) {
    walk<kPf>(base, lane, n, M, r0, zero, [](int) {}, body, tail);
}

// The wavefront's maximum in every lane.  No operand is ever a NaN, so the order of a maximum does not matter.
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = fmaxf(x, __shfl_xor(x, d));
    return x;
}

// The contract's halving fold of 64 fp64 partials, one per lane, into lane 0: p_j += p_{j+w} for j < w, w = 32 ... 1; partial j + w
// sits w lanes up (the lanes from w up hold nothing that is used).  Several sums fold side by side.
template <typename... D>
__device__ __forceinline__ void fold(D&... p) {
#pragma unroll
    for (int w = kT / 2; w >= 1; w >>= 1) ((p += __shfl_down(p, w)), ...);
}

// neither inf nor NaN
__device__ __forceinline__ bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// One hysteresis detector's step at an interval's end (lane 0), on its counters in the station's record: bit k of `flags` is raised
// after `raise` intervals in a row with `hit` and cleared after `clear` in a row without.  Returns the flags.
__device__ __forceinline__ unsigned detect(unsigned flags, int k, bool hit, int raise, int clear, unsigned& run_k, unsigned& transitions_k) {
    const unsigned bit = 1u << k;
    unsigned run = run_k;
    if (!(flags & bit)) {
        run = hit ? run + 1 : 0;
        if (run >= (unsigned)raise) { flags |= bit; run = 0; transitions_k++; }
    } else {
        run = hit ? 0 : run + 1;
        if (run >= (unsigned)clear) { flags &= ~bit; run = 0; transitions_k++; }
    }
    run_k = run;
    return flags;
}

}  // namespace rows
}  // namespace fmd
