// The row map of the batched objects whose stations hand over uneven numbers of rows a call (the fingerprinter's sub-blocks, the
// matcher's queries), stated once.  Device code; included by fmd_fprint.hip and fmd_fpmatch.hip only.
//
// Geometry: station c contributes count(c) >= 0 rows, and its rows are base[c] ... base[c + 1] - 1 of the batch, base [C + 1] the
// exclusive prefix sum of the counts, base[C] the batch's rows.  The forward map is ONE workgroup of kThreads = 1024: thread t takes the
// contiguous share of ceil(C / 1024) stations from t * ceil(C / 1024) on (short or empty behind C), the shares' sums are scanned in LDS
// (Hillis-Steele, 10 steps), and every thread replays its share's counts from its exclusive sum; thread 1023 holds the total.  The
// inverse is a bisection over base.  All integer, so the map is the same whatever the geometry.
#pragma once
#include <hip/hip_runtime.h>

namespace fmd {
namespace rowmap {

constexpr int kThreads = 1024;       // the forward map's workgroup; a kernel that calls scan() is launched as <<<1, kThreads>>>

// base[0 ... C]: the exclusive prefix sum of count(0) ... count(C - 1).  Every thread of the workgroup calls it (barriers inside);
// count(c) is called twice per station, with c in [0, C), and must give the same value both times.
template <typename Count>
__device__ __forceinline__ void scan(int C, Count&& count, int* __restrict__ base) {
    __shared__ int part[kThreads];
    const int tid = threadIdx.x;
    const int per = (C + kThreads - 1) / kThreads;
    const int c0 = min(tid * per, C), c1 = min(c0 + per, C);
    int sum = 0;
    for (int c = c0; c < c1; c++) sum += count(c);
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int c = c0; c < c1; c++) {
        base[c] = run;
        run += count(c);
    }
    if (tid == kThreads - 1) base[C] = part[tid];
}

// The largest i in [0, n) with base[i] <= r, base ascending (not strictly).  The caller sees to n >= 1 and base[0] <= r, otherwise 0
// comes back whatever base[0] is.  With base a scan()'s output and r a row in [0, base[n]), i is the station the row belongs to:
// base[i] <= r < base[i + 1] (a station of no rows is never the largest).  With base a catalogue's track starts [T + 1], starts[0] = 0,
// and r a position in [0, starts[T]), i is the position's track.  Reads base[1 ... n - 1] only.
__device__ __forceinline__ int owner(const int* __restrict__ base, int n, int r) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace rowmap
}  // namespace fmd
