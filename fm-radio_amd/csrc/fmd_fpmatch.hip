// Fingerprint matcher, device side (include/fmdemod.h, "Fingerprint matcher").
//
// NOT in the reference.  Per station a ring of its newest W fingerprint words; whenever the station's word count crosses a multiple of
// the interval, its newest W words against every valid position of the catalogue: errs = sum popcount((q ^ cat) & mask), the smallest,
// on a tie the lowest position.  All integer, so every tiling gives the same result.
//
// Four kernels a call:
//   k_fpmatch_map     one workgroup: the queries each active station fires, as an exclusive prefix sum: the rows of the search.  The scan
//                     and its inverse (row -> station, and position -> track over the starts table) are fmd_rowmap.h's, shared with
//                     the fingerprinter.
//   k_fpmatch_gather  a workgroup a query: its W words, masked, from the ring and the caller's new words into a contiguous window.
//   k_fpmatch_search  queries x catalogue positions with depth W.  A workgroup holds kFpmatchQueries queries and walks the column tiles
//                     of its column group: the tile's kFpmatchTile + W - 1 catalogue words are staged once in LDS, lane <-> position
//                     (lane p reads word p + j: consecutive lanes, consecutive banks), the queries' words are wave-uniform and come
//                     through scalar loads, and a step is one XOR and one accumulating population count a query.  The minimum is the
//                     packed key errs << 32 | p, so an unsigned minimum is the tie rule; it is carried in registers over the group's
//                     tiles, reduced across lanes by shuffles and across the four wavefronts through LDS, and written as the group's
//                     partial minimum.
//   k_fpmatch_finish  a wavefront a station: per query the minimum over the groups' partials, the track from the starts table, the
//                     detector, the event; then the ring's newest words, the record, the count and the bytes.  All but the first step is
//                     fpm_finish, stated once for both finish kernels: a kernel is the source of a row's key, handed in as a hook.
// An indexed object (fmd_fpmatch_create_ex) keeps map and gather and puts two kernels of its own behind them:
//   k_fpmatch_probe       a workgroup a query.  Lane <-> window word j: the directory slice of the word's key, a binary search for the
//                         key's run in the sorted keys, runs longer than K skipped.  A run's positions p' propose p = p' - j; a proposal
//                         inside [0, D - W] that the workgroup's LDS set has not seen goes into the LDS list, so a position most of the W
//                         look-ups agree on is counted once.  The window is walked in chunks of chunk_words words so that a chunk's
//                         runs fit the list.  Then a wavefront (16 lanes where W < 64) a listed position: track validity, and the W
//                         catalogue words at p read by consecutive lanes against the window in LDS, XOR, population count, a shuffle
//                         sum.  The packed minimum as in the search; one partial a row, and the row's (candidates, skipped) counts.
//   k_fpmatch_finish_idx  fpm_finish with the indexed object's key: the row's one partial and, counted here before the query's detector
//                         step, the follow rule's 2 d + 1 positions around the expected one, because they depend on the detector state
//                         the query before left; adds the row's counts to the station's index record.
// No global atomics (the probe's set and list use LDS atomics inside one workgroup), no register spills (scratch 0), no workgroup waits
// on another, ordinary vector stores only.
//
// Bounds: k_fpmatch_gather reads ring slots taken mod W, new words below the station's k <= n <= words_stride, and writes window rows
// below qbase[C] <= C * max_events(I, n) <= max_queries.  k_fpmatch_search reads catalogue words below D (zero behind it), LDS words below
// kFpmatchTile - 1 + W - 1 < lds_words, starts entries 0 ... T, window rows below qbase[C] (a row past the last repeats it) and writes
// partials at row * G + group, group < G <= groups.  fpm_finish (both finish kernels) writes events below the station's count <= max_events(I, n) <=
// events_stride and ring slots mod W.  k_fpmatch_probe reads window row r < qbase[C], directory entries b and b + 1 with b = key >> (32 -
// dir_bits) < 2^dir_bits (the directory holds 2^dir_bits + 1), keys and positions at dir[b] ... dir[b + 1] - 1 < D, s_win below W <= 1024;
// a chunk lists at most chunk_words * K <= kFpmIndexChunk positions (chunk_words = min(256, kFpmIndexChunk / K): W = 1024 at K = 64 is 16
// chunks of 64 words), each in [0, D - W], so the catalogue words p ... p + W - 1 lie below D; the set holds at most 3/4 of its
// kFpmIndexTable slots (it is emptied before a chunk that could take it above that), so a probe sequence ends; starts entries 0 ... T.
// k_fpmatch_finish_idx counts only positions in [0, D - W] whose W words lie inside one track, from window row row0 + i < qbase[C].
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fmd_fpmatch_design.h"
#include "fmd_fpmatch_index.h"
#include "fmd_rowmap.h"
#include "fmd_side.h"
#include "fmdemod.h"

using fmd::FpmatchLayout;
using fmd::kFpmatchQueries;
using fmd::kFpmatchThreads;
using fmd::kFpmatchTile;
using fmd::kFpmIndexChunk;
using fmd::kFpmIndexTable;
using fmd::kFpmIndexThreads;
using fmd::rowmap::owner;               // the track of a position (starts [T + 1]) and the station of a row (qbase [C + 1])

namespace {

constexpr int kQR = kFpmatchQueries;
constexpr int kWaves = kFpmatchThreads / 64;
constexpr int kPasses = kFpmatchTile / kFpmatchThreads;
constexpr unsigned long long kNoKey = ~0ull;
static_assert(kFpmatchTile % kFpmatchThreads == 0, "a tile is whole passes of a workgroup");

static_assert(sizeof(fmd_fpmatch_status) == 64 && offsetof(fmd_fpmatch_status, since) == 32 && offsetof(fmd_fpmatch_status, track) == 40 &&
              offsetof(fmd_fpmatch_status, errs) == 48 && offsetof(fmd_fpmatch_status, flags) == 60, "fmd_fpmatch_status layout");
static_assert(sizeof(fmd_fpmatch_index_status) == 32 && offsetof(fmd_fpmatch_index_status, empty) == 24, "fmd_fpmatch_index_status layout");
static_assert(kFpmIndexThreads == kFpmatchThreads && (kFpmIndexTable & (kFpmIndexTable - 1)) == 0, "the probe's workgroup and set");
static_assert(sizeof(fmd_fpmatch_event) == 24 && offsetof(fmd_fpmatch_event, track) == 8 && offsetof(fmd_fpmatch_event, errs) == 16, "fmd_fpmatch_event layout");

// what the kernels read of the configuration
struct FpmDev {
    int C, W, I, hold;
    unsigned max_errs, mask;
};

// what k_fpmatch_probe and k_fpmatch_finish_idx read of the index: keys [D] ascending, pos [D], dir [2^dir_bits + 1]
struct FpmIdxDev {
    const uint32_t* keys;
    const int* pos;
    const int* dir;
    int dir_bits, K, chunk_words, follow;
};

// ---- the pieces a later object (station against station) can reuse: the take, the query schedule, the ring and the error count

// the words station c hands over: d_nwords[c] clamped into [0, n]
__device__ __forceinline__ int fpm_take(const int* __restrict__ nwords, int c, int n, bool* clamped) {
    *clamped = false;
    if (!nwords) return n;
    const int k = nwords[c];
    *clamped = k < 0 || k > n;
    return k < 0 ? 0 : (k > n ? n : k);
}

// the queries of a station that had `before` words and takes k: their number, and the first one's e
__device__ __forceinline__ int fpm_queries(unsigned long long before, int k, int W, int I, unsigned long long* e0) {
    const unsigned long long after = before + (unsigned long long)k;
    const unsigned long long m = before > (unsigned long long)(W - 1) ? before : (unsigned long long)(W - 1);   // e > m
    *e0 = (m / (unsigned long long)I + 1ull) * (unsigned long long)I;
    const long long cnt = (long long)(after / (unsigned long long)I) - (long long)(m / (unsigned long long)I);
    return cnt > 0 ? (int)cnt : 0;
}

// word i of a station (counted from its reset): in the ring [W] where the station had it before this call, else among the new words
__device__ __forceinline__ uint32_t fpm_word(const uint32_t* __restrict__ ring, const uint32_t* __restrict__ fresh, int W, unsigned long long before,
                                             unsigned long long i) {
    return i < before ? ring[(int)(i % (unsigned long long)W)] : fresh[(size_t)(i - before)];
}

// errs += popcount(q ^ c), both masked already: v_xor_b32, v_bcnt_u32_b32
__device__ __forceinline__ unsigned fpm_errs(unsigned errs, uint32_t q, uint32_t c) { return (unsigned)__builtin_popcount(q ^ c) + errs; }

__device__ __forceinline__ unsigned long long fpm_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// the minimum over the wavefront, in every lane
__device__ __forceinline__ unsigned long long fpm_wave_min(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, 64);
        v = fpm_min(v, ((unsigned long long)hi << 32) | lo);
    }
    return v;
}

// qbase [C + 1]: the exclusive prefix sum of the queries each active station fires
__global__ __launch_bounds__(fmd::rowmap::kThreads) void k_fpmatch_map(FpmDev g, int n, const int* __restrict__ nwords, const uint8_t* __restrict__ active,
                                                                      const fmd_fpmatch_status* __restrict__ status, int* __restrict__ qbase) {
    auto count = [&](int c) {
        if (active && active[c] == 0) return 0;
        bool cl;
        unsigned long long e0;
        return fpm_queries(status[c].words, fpm_take(nwords, c, n, &cl), g.W, g.I, &e0);
    };
    fmd::rowmap::scan(g.C, count, qbase);
}

// qwin [rows][W]: row r's window, masked
__global__ __launch_bounds__(64) void k_fpmatch_gather(FpmDev g, int n, const int* __restrict__ nwords, const fmd_fpmatch_status* __restrict__ status,
                                                      const int* __restrict__ qbase, const uint32_t* __restrict__ ring_all, const uint32_t* __restrict__ words,
                                                      long long words_stride, uint32_t* __restrict__ qwin) {
    const int r = blockIdx.x;
    if (r >= qbase[g.C]) return;                                             // surplus workgroups leave at once
    const int c = owner(qbase, g.C, r);                                      // qbase[c] <= r < qbase[c + 1]
    const unsigned long long before = status[c].words;
    bool cl;
    unsigned long long e0;
    (void)fpm_queries(before, fpm_take(nwords, c, n, &cl), g.W, g.I, &e0);
    const unsigned long long e = e0 + (unsigned long long)(r - qbase[c]) * (unsigned long long)g.I;
    const uint32_t* ring = ring_all + (size_t)c * (size_t)g.W;
    const uint32_t* fresh = words + (size_t)c * (size_t)words_stride;
    for (int j = threadIdx.x; j < g.W; j += 64)
        qwin[(size_t)r * (size_t)g.W + j] = fpm_word(ring, fresh, g.W, before, e - (unsigned long long)g.W + (unsigned long long)j) & g.mask;
}

// cat [D], masked; starts [T + 1]; part [rows][G]
__global__ __launch_bounds__(kFpmatchThreads) void k_fpmatch_search(int C, int W, const int* __restrict__ qbase, const uint32_t* __restrict__ qwin,
                                                                   const uint32_t* __restrict__ cat, int D, const int* __restrict__ starts, int T, int G,
                                                                   unsigned long long* __restrict__ part) {
    extern __shared__ uint32_t s_cat[];                                      // [kFpmatchTile + W - 1]
    __shared__ unsigned long long s_red[kWaves][kQR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Q = qbase[C];
    const int r0 = blockIdx.x * kQR;
    if (r0 >= Q) return;                                                     // surplus workgroups leave at once (uniform)
    const int npos = D - W + 1, ntiles = (npos + kFpmatchTile - 1) / kFpmatchTile;
    const uint32_t* qp[kQR];
#pragma unroll
    for (int r = 0; r < kQR; r++) qp[r] = qwin + (size_t)min(r0 + r, Q - 1) * (size_t)W;   // a row past the last repeats it
    unsigned long long best[kQR];
#pragma unroll
    for (int r = 0; r < kQR; r++) best[r] = kNoKey;

    for (int t = blockIdx.y; t < ntiles; t += G) {
        const int base = t * kFpmatchTile;
        __syncthreads();                                                     // the tile before is read
        for (int i = tid; i < kFpmatchTile + W - 1; i += kFpmatchThreads) s_cat[i] = base + i < D ? cat[base + i] : 0u;
        __syncthreads();
        for (int s = 0; s < kPasses; s++) {
            const int pl = s * kFpmatchThreads + wave * 64 + lane, p = base + pl;
            bool valid = p < npos;
            if (valid) {
                const int tr = owner(starts, T, p);
                valid = p + W <= starts[tr + 1];
            }
            if (!__any(valid)) continue;                                     // (per wavefront; no barrier inside)
            unsigned acc[kQR];
#pragma unroll
            for (int r = 0; r < kQR; r++) acc[r] = 0u;
            const uint32_t* cp = s_cat + pl;
            for (int j0 = 0; j0 < W; j0 += 8) {
#pragma unroll
                for (int jj = 0; jj < 8; jj++) {
                    const uint32_t cw = cp[j0 + jj];
#pragma unroll
                    for (int r = 0; r < kQR; r++) acc[r] = fpm_errs(acc[r], qp[r][j0 + jj], cw);
                }
            }
            if (valid) {
#pragma unroll
                for (int r = 0; r < kQR; r++) best[r] = fpm_min(best[r], ((unsigned long long)acc[r] << 32) | (unsigned)p);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kQR; r++) {
        const unsigned long long m = fpm_wave_min(best[r]);
        if (lane == 0) s_red[wave][r] = m;
    }
    __syncthreads();
    if (tid < kQR && r0 + tid < Q) {
        unsigned long long m = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < kWaves; w++) m = fpm_min(m, s_red[w][tid]);
        part[(size_t)(r0 + tid) * (size_t)G + blockIdx.y] = m;
    }
}

// The finish of a call, stated once for both objects: a wavefront a station (the caller has seen to `active`).  Walks the station's
// queries in order: key(row, st) is the row's packed minimum errs << 32 | p, or kNoKey, called with the record st as the query before
// left it and the same in every lane; then the key as (track, offset, errs), the detector's step, the event.  Behind the walk, when every
// reader of the ring and of the windows is done (k_fpmatch_gather and whatever key() reads): the ring's newest words, the record, the
// count and the bytes.  key's state is the caller's locals.
template <typename Key>
__device__ __forceinline__ void fpm_finish(const FpmDev& g, int c, int lane, int n, const int* __restrict__ nwords, const int* __restrict__ qbase,
                                           const int* __restrict__ starts, int T, const uint32_t* __restrict__ words, long long words_stride,
                                           fmd_fpmatch_status* __restrict__ status, uint32_t* __restrict__ ring_all, fmd_fpmatch_event* __restrict__ events,
                                           long long events_stride, int* __restrict__ nevents, uint8_t* __restrict__ flags, uint8_t* __restrict__ ok, Key&& key) {
    fmd_fpmatch_status st = status[c];
    const unsigned long long before = st.words;
    bool clamped;
    const int k = fpm_take(nwords, c, n, &clamped);
    unsigned long long e0;
    const int cnt = fpm_queries(before, k, g.W, g.I, &e0);
    const int row0 = qbase[c];
    // every lane walks the detector alike; lane 0 stores
    for (int i = 0; i < cnt; i++) {
        const unsigned long long m = key(row0 + i, st);
        const unsigned long long e = e0 + (unsigned long long)i * (unsigned long long)g.I;
        int track = -1, offset = 0;
        unsigned errs = 0xffffffffu;
        if (m != kNoKey) {
            const int p = (int)(unsigned)m;
            errs = (unsigned)(m >> 32);
            track = owner(starts, T, p);
            offset = p - starts[track];
        }
        const bool hit = track >= 0 && errs <= g.max_errs;
        st.queries += 1;
        st.errs = errs;
        if (hit) {
            st.hits += 1;
            if (st.track != track) { st.track = track; st.since = e; }
            st.offset = offset;
            st.misses = 0;
        } else if (st.track >= 0) {
            st.misses += 1;
            if (st.misses == (unsigned)g.hold) { st.track = -1; st.misses = 0; }
        }
        st.flags = hit ? 2u : 0u;
        if (lane == 0) {
            fmd_fpmatch_event ev;
            ev.end = e; ev.track = track; ev.offset = offset; ev.errs = errs; ev.flags = hit ? 1u : 0u;
            events[(size_t)c * (size_t)events_stride + (size_t)i] = ev;
        }
    }
    // the ring's newest words: of the k new ones the last min(k, W)
    uint32_t* ring = ring_all + (size_t)c * (size_t)g.W;
    for (int j = (k > g.W ? k - g.W : 0) + lane; j < k; j += 64)
        ring[(int)((before + (unsigned long long)j) % (unsigned long long)g.W)] = words[(size_t)c * (size_t)words_stride + (size_t)j];
    if (lane == 0) {
        st.words = before + (unsigned long long)k;
        st.clamped += clamped ? 1ull : 0ull;
        st.fill = st.words < (unsigned long long)g.W ? (unsigned)st.words : (unsigned)g.W;
        st.flags = (st.flags & 2u) | (st.track >= 0 ? 1u : 0u);
        status[c] = st;
        if (nevents) nevents[c] = cnt;
        if (flags) flags[c] = (uint8_t)st.flags;
        if (ok) ok[c] = (uint8_t)(st.flags & 1u);
    }
}

// a wavefront a station: a row's key is the minimum over its G partials; G = 0 with an empty catalogue
__global__ __launch_bounds__(64) void k_fpmatch_finish(FpmDev g, int n, const int* __restrict__ nwords, const uint8_t* __restrict__ active, const int* __restrict__ qbase,
                                                      const unsigned long long* __restrict__ part, int G, const int* __restrict__ starts, int T,
                                                      const uint32_t* __restrict__ words, long long words_stride, fmd_fpmatch_status* __restrict__ status,
                                                      uint32_t* __restrict__ ring_all, fmd_fpmatch_event* __restrict__ events, long long events_stride,
                                                      int* __restrict__ nevents, uint8_t* __restrict__ flags, uint8_t* __restrict__ ok) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (active && active[c] == 0) return;
    fpm_finish(g, c, lane, n, nwords, qbase, starts, T, words, words_stride, status, ring_all, events, events_stride, nevents, flags, ok,
               [&](int row, const fmd_fpmatch_status&) {
                   unsigned long long key = kNoKey;
                   for (int y = lane; y < G; y += 64) key = fpm_min(key, part[(size_t)row * (size_t)G + y]);
                   return fpm_wave_min(key);
               });
}

// whether position p, inside [0, D - W], has its W words inside one track
__device__ __forceinline__ bool fpm_valid(const int* __restrict__ starts, int T, int p, int W) { return p + W <= starts[owner(starts, T, p) + 1]; }

// the sum over groups of L consecutive lanes (L = 16 or 64), in every lane of the group
template <int L>
__device__ __forceinline__ unsigned fpm_group_sum(unsigned v) {
#pragma unroll
    for (int d = L / 2; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

// the listed positions s_list[0 ... n - 1] against the window: L lanes a position, 64 / L positions a wavefront at once
template <int L>
__device__ __forceinline__ unsigned long long fpm_count_list(const int* s_list, int n, const uint32_t* s_win, int W, const uint32_t* __restrict__ cat,
                                                             const int* __restrict__ starts, int T, unsigned long long best) {
    constexpr int per = 64 / L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / L, l = lane % L;
    for (int i0 = 0; i0 < n; i0 += kWaves * per) {                           // (uniform bounds: every lane reaches the shuffles)
        const int i = i0 + wave * per + g;
        const int p = i < n ? s_list[i] : 0;
        const bool valid = i < n && fpm_valid(starts, T, p, W);
        unsigned e = 0u;
        if (valid)
            for (int j = l; j < W; j += L) e = fpm_errs(e, s_win[j], cat[(size_t)p + (size_t)j]);
        e = fpm_group_sum<L>(e);
        if (valid) best = fpm_min(best, ((unsigned long long)e << 32) | (unsigned)p);
    }
    return best;
}

// part [rows]: the row's minimum over its look-ups' valid positions; rowstat [rows]: (candidates, skipped)
__global__ __launch_bounds__(kFpmIndexThreads) void k_fpmatch_probe(int C, int W, const int* __restrict__ qbase, const uint32_t* __restrict__ qwin,
                                                                   const uint32_t* __restrict__ cat, int D, const int* __restrict__ starts, int T, FpmIdxDev x,
                                                                   unsigned long long* __restrict__ part, uint2* __restrict__ rowstat) {
    __shared__ uint32_t s_win[1024];                                         // the window (W <= 1024)
    __shared__ int s_list[kFpmIndexChunk];                                   // the chunk's positions, each once
    __shared__ int s_tab[kFpmIndexTable];                                    // the set of the positions listed so far, open addressing, -1 = free
    __shared__ int s_n;                                                      // positions in the list
    __shared__ unsigned long long s_red[kWaves];
    __shared__ unsigned s_cnt[kWaves][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    if (r >= qbase[C]) return;                                               // surplus workgroups leave at once (uniform)
    for (int j = tid; j < W; j += kFpmIndexThreads) s_win[j] = qwin[(size_t)r * (size_t)W + j];
    for (int i = tid; i < kFpmIndexTable; i += kFpmIndexThreads) s_tab[i] = -1;
    if (tid == 0) s_n = 0;
    int fill = 0;                                                            // the set's entries (uniform)
    unsigned long long best = kNoKey;
    unsigned cand = 0u, skip = 0u;
    __syncthreads();
    for (int j0 = 0; j0 < W; j0 += x.chunk_words) {
        if (fill + x.chunk_words * x.K > kFpmIndexTable / 4 * 3) {           // the set could pass 3/4: emptied (repeats of earlier chunks are then counted again)
            for (int i = tid; i < kFpmIndexTable; i += kFpmIndexThreads) s_tab[i] = -1;
            fill = 0;
            __syncthreads();
        }
        const int j = j0 + tid;
        if (tid < x.chunk_words && j < W) {
            const uint32_t k = s_win[j];
            const unsigned b = k >> (32 - x.dir_bits);
            const int hi = x.dir[b + 1];
            int a = x.dir[b], z = hi;
            while (a < z) {                                                  // the first key >= k of the slice
                const int mid = (a + z) >> 1;
                if (x.keys[mid] < k) a = mid + 1; else z = mid;
            }
            const int first = a;
            z = min(hi, first + x.K + 1);
            while (a < z) {                                                  // the first key > k among the K + 1 behind it
                const int mid = (a + z) >> 1;
                if (x.keys[mid] <= k) a = mid + 1; else z = mid;
            }
            const int run = a - first;
            if (run > x.K) {
                skip += 1u;
            } else {
                cand += (unsigned)run;
                for (int i = first; i < first + run; i++) {
                    const int p = x.pos[i] - j;
                    if (p < 0 || p > D - W) continue;
                    unsigned h = ((unsigned)p * 2654435761u) >> 19;          // 13 bits
                    static_assert(kFpmIndexTable == 1 << 13, "the hash's width");
                    for (;;) {
                        const int old = atomicCAS(&s_tab[h], -1, p);
                        if (old == -1) { s_list[atomicAdd(&s_n, 1)] = p; break; }
                        if (old == p) break;
                        h = (h + 1u) & (unsigned)(kFpmIndexTable - 1);
                    }
                }
            }
        }
        __syncthreads();
        const int n = s_n;
        best = W >= 64 ? fpm_count_list<64>(s_list, n, s_win, W, cat, starts, T, best) : fpm_count_list<16>(s_list, n, s_win, W, cat, starts, T, best);
        fill += n;
        __syncthreads();                                                     // the list is read
        if (tid == 0) s_n = 0;
        __syncthreads();
    }
    best = fpm_wave_min(best);
    cand = fpm_group_sum<64>(cand);
    skip = fpm_group_sum<64>(skip);
    if (lane == 0) { s_red[wave] = best; s_cnt[wave][0] = cand; s_cnt[wave][1] = skip; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = s_red[0];
        uint2 cs = make_uint2(s_cnt[0][0], s_cnt[0][1]);
#pragma unroll
        for (int w = 1; w < kWaves; w++) { m = fpm_min(m, s_red[w]); cs.x += s_cnt[w][0]; cs.y += s_cnt[w][1]; }
        part[r] = m;
        rowstat[r] = cs;
    }
}

// k_fpmatch_finish for the indexed object: a row's key is its one partial and the follow rule's positions, counted here against the
// detector state the query before left; the row's counts go to the station's index record.  probed = 0 with an empty catalogue (no
// rows were probed)
__global__ __launch_bounds__(64) void k_fpmatch_finish_idx(FpmDev g, int n, const int* __restrict__ nwords, const uint8_t* __restrict__ active, const int* __restrict__ qbase,
                                                          const unsigned long long* __restrict__ part, const uint2* __restrict__ rowstat, int probed,
                                                          const uint32_t* __restrict__ qwin, const uint32_t* __restrict__ cat, int D, int follow,
                                                          const int* __restrict__ starts, int T, const uint32_t* __restrict__ words, long long words_stride,
                                                          fmd_fpmatch_status* __restrict__ status, fmd_fpmatch_index_status* __restrict__ istatus,
                                                          uint32_t* __restrict__ ring_all, fmd_fpmatch_event* __restrict__ events, long long events_stride,
                                                          int* __restrict__ nevents, uint8_t* __restrict__ flags, uint8_t* __restrict__ ok) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (active && active[c] == 0) return;
    fmd_fpmatch_index_status ix = istatus[c];
    fpm_finish(g, c, lane, n, nwords, qbase, starts, T, words, words_stride, status, ring_all, events, events_stride, nevents, flags, ok,
               [&](int row, const fmd_fpmatch_status& st) {
                   unsigned long long key = kNoKey;
                   if (probed) {
                       key = part[row];
                       const uint2 cs = rowstat[row];
                       ix.candidates += cs.x;
                       ix.skipped += cs.y;
                   }
                   if (follow > 0 && st.track >= 0) {                        // (identified: the catalogue is not empty, since a load clears the track)
                       ix.followed += 1ull;
                       const long long p_exp = (long long)starts[st.track] + (long long)st.offset + (long long)g.I * ((long long)st.misses + 1ll);
                       const uint32_t* q = qwin + (size_t)row * (size_t)g.W;
                       for (long long p = p_exp - follow; p <= p_exp + follow; p++) {   // (uniform: every lane reaches the shuffles)
                           if (p < 0 || p > (long long)(D - g.W) || !fpm_valid(starts, T, (int)p, g.W)) continue;
                           unsigned e = 0u;
                           for (int j = lane; j < g.W; j += 64) e = fpm_errs(e, q[j], cat[(size_t)p + (size_t)j]);
                           e = fpm_group_sum<64>(e);
                           key = fpm_min(key, ((unsigned long long)e << 32) | (unsigned)p);
                       }
                   }
                   if (key == kNoKey) ix.empty += 1ull;
                   return key;
               });
    if (lane == 0) istatus[c] = ix;
}

// stations c0 ... as after create
__global__ __launch_bounds__(64) void k_fpmatch_reset(int c0, int cn, fmd_fpmatch_status* __restrict__ status) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= cn) return;
    fmd_fpmatch_status z{};
    z.track = -1;
    status[c0 + i] = z;
}

// a new catalogue: every station's detector cleared, the catalogue's words masked in place
__global__ __launch_bounds__(256) void k_fpmatch_loaded(int C, fmd_fpmatch_status* __restrict__ status, uint32_t* __restrict__ cat, int D, unsigned mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < C) {
        status[i].track = -1;
        status[i].misses = 0u;
        status[i].flags &= 2u;
    }
    if (i < D) cat[i] &= mask;
}

}  // namespace

struct fmd_fpmatch_s {
    fmd_fpmatch_config cfg{};
    FpmatchLayout lay{};
    FpmDev dev{};
    int D = 0, T = 0;                              // the catalogue's words and tracks
    fmd_fpmatch_status* d_status = nullptr;        // [C]
    uint32_t* d_ring = nullptr;                    // [C][W]: word i lies in slot i mod W
    uint32_t* d_cat = nullptr;                     // [max_catalogue_words], masked
    int* d_starts = nullptr;                       // [max_tracks + 1]
    int* d_qbase = nullptr;                        // [C + 1]
    uint32_t* d_qwin = nullptr;                    // [max_queries][W]
    unsigned long long* d_part = nullptr;          // [max_queries][groups]; indexed: [max_queries]
    // an indexed object (fmd_fpmatch_create_ex) only
    bool indexed = false;
    fmd_fpmatch_index_config icfg{};
    fmd::FpmIndexLayout ilay{};
    uint32_t* d_keys = nullptr;                    // [max_catalogue_words]: the masked words ascending
    int* d_pos = nullptr;                          // [max_catalogue_words]: their positions
    int* d_dir = nullptr;                          // [2^dir_bits + 1]
    uint2* d_rowstat = nullptr;                    // [max_queries]: (candidates, skipped) of a row
    fmd_fpmatch_index_status* d_istatus = nullptr; // [C]
    fmd::CallOrder order;
    std::string err;
};

template <typename... A>
static int fpm_fail(fmd_fpmatch h, int code, const char* fmt, A... args) { return fmd::fail(h ? h->err : fmd::fpmatch_global_error(), code, fmt, args...); }

extern "C" {

int fmd_fpmatch_create(const fmd_fpmatch_config* cfg, fmd_fpmatch* out) { return fmd_fpmatch_create_ex(cfg, nullptr, out); }

int fmd_fpmatch_create_ex(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx, fmd_fpmatch* out) {
    if (!cfg || !out) return fpm_fail(nullptr, FMD_ERR_ARG, "null configuration or handle");
    std::string why;
    if (fmd::fpmatch_check(cfg, &why) != FMD_OK || (idx && fmd::fpmatch_index_check(idx, &why) != FMD_OK)) return fpm_fail(nullptr, FMD_ERR_ARG, "%s", why.c_str());
    if (fmd_device_count() <= 0) return fpm_fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return fpm_fail(nullptr, FMD_ERR_DEVICE, "hipGetDevice failed");
    fmd_fpmatch h = new fmd_fpmatch_s();
    h->cfg = *cfg;
    h->lay = fmd::fpmatch_layout(cfg);
    h->dev = FpmDev{cfg->n_channels, cfg->block, cfg->interval, cfg->hold, (unsigned)cfg->max_errs, h->lay.mask};
    const size_t C = (size_t)cfg->n_channels, W = (size_t)cfg->block, Qm = (size_t)h->lay.max_queries;
    if (idx) {
        h->indexed = true;
        h->icfg = *idx;
        h->ilay = fmd::fpmatch_index_layout(cfg, idx);
    }
    const size_t parts = idx ? 1 : (size_t)h->lay.groups;
    bool ok = h->order.init(dev);
    ok = ok && hipMalloc(&h->d_status, sizeof(fmd_fpmatch_status) * C) == hipSuccess;
    ok = ok && hipMalloc(&h->d_ring, sizeof(uint32_t) * C * W) == hipSuccess;
    ok = ok && hipMalloc(&h->d_cat, sizeof(uint32_t) * (size_t)cfg->max_catalogue_words) == hipSuccess;
    ok = ok && hipMalloc(&h->d_starts, sizeof(int) * ((size_t)cfg->max_tracks + 1)) == hipSuccess;
    ok = ok && hipMalloc(&h->d_qbase, sizeof(int) * (C + 1)) == hipSuccess;
    ok = ok && hipMalloc(&h->d_qwin, sizeof(uint32_t) * Qm * W) == hipSuccess;
    ok = ok && hipMalloc(&h->d_part, sizeof(unsigned long long) * Qm * parts) == hipSuccess;
    ok = ok && hipMemset(h->d_starts, 0, sizeof(int) * ((size_t)cfg->max_tracks + 1)) == hipSuccess;
    if (idx) {
        ok = ok && hipMalloc(&h->d_keys, sizeof(uint32_t) * (size_t)cfg->max_catalogue_words) == hipSuccess;
        ok = ok && hipMalloc(&h->d_pos, sizeof(int) * (size_t)cfg->max_catalogue_words) == hipSuccess;
        ok = ok && hipMalloc(&h->d_dir, sizeof(int) * (size_t)h->ilay.dir_entries) == hipSuccess;
        ok = ok && hipMalloc(&h->d_rowstat, sizeof(uint2) * Qm) == hipSuccess;
        ok = ok && hipMalloc(&h->d_istatus, sizeof(fmd_fpmatch_index_status) * C) == hipSuccess;
        ok = ok && hipMemset(h->d_dir, 0, sizeof(int) * (size_t)h->ilay.dir_entries) == hipSuccess;
    }
    if (!ok || fmd_fpmatch_reset(h, -1) != FMD_OK) {
        const long long bytes = idx ? h->ilay.bytes : h->lay.bytes;
        (void)hipGetLastError();
        fmd_fpmatch_destroy(h);
        return fpm_fail(nullptr, FMD_ERR_DEVICE, "device allocation of %lld bytes failed", bytes);
    }
    *out = h;
    return FMD_OK;
}

int fmd_fpmatch_destroy(fmd_fpmatch h) {
    if (!h) return FMD_ERR_ARG;
    (void)h->order.quiesce();
    for (void* p : {(void*)h->d_status, (void*)h->d_ring, (void*)h->d_cat, (void*)h->d_starts, (void*)h->d_qbase, (void*)h->d_qwin, (void*)h->d_part,
                    (void*)h->d_keys, (void*)h->d_pos, (void*)h->d_dir, (void*)h->d_rowstat, (void*)h->d_istatus})
        if (p) (void)hipFree(p);
    delete h;
    return FMD_OK;
}

int fmd_fpmatch_reset(fmd_fpmatch h, int channel) {
    if (!h) return FMD_ERR_ARG;
    int c0, cn;
    if (!fmd::channel_range(channel, h->cfg.n_channels, &c0, &cn)) return fpm_fail(h, FMD_ERR_ARG, "channel %d outside [-1, %d)", channel, h->cfg.n_channels);
    if (!h->order.quiesce()) return fpm_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    hipLaunchKernelGGL(k_fpmatch_reset, dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, nullptr, c0, cn, h->d_status);
    if (h->indexed && hipMemsetAsync(h->d_istatus + c0, 0, sizeof(fmd_fpmatch_index_status) * (size_t)cn, nullptr) != hipSuccess)
        return fpm_fail(h, FMD_ERR_DEVICE, "clearing the index records failed");
    if (const char* e = fmd::control_end("k_fpmatch_reset launch failed")) return fpm_fail(h, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_fpmatch_load(fmd_fpmatch h, const uint32_t* words, const long long* starts, int n_tracks) {
    if (!h) return FMD_ERR_ARG;
    std::string why;
    if (fmd::fpmatch_check_catalogue(&h->cfg, starts, n_tracks, &why) != FMD_OK) return fpm_fail(h, FMD_ERR_ARG, "%s", why.c_str());
    const long long D = n_tracks > 0 ? starts[n_tracks] : 0;
    if (D > 0 && !words) return fpm_fail(h, FMD_ERR_ARG, "null words");
    if (!h->order.quiesce()) return fpm_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    if (h->indexed) {                                                        // the index of the new catalogue, built here on the host
        std::vector<uint32_t> keys((size_t)D);
        std::vector<int32_t> pos((size_t)D), dir((size_t)h->ilay.dir_entries);
        fmd::fpmatch_index_build(words, D, h->lay.mask, h->ilay.dir_bits, keys.data(), pos.data(), dir.data());
        if ((D > 0 && (hipMemcpy(h->d_keys, keys.data(), sizeof(uint32_t) * (size_t)D, hipMemcpyHostToDevice) != hipSuccess ||
                       hipMemcpy(h->d_pos, pos.data(), sizeof(int) * (size_t)D, hipMemcpyHostToDevice) != hipSuccess)) ||
            hipMemcpy(h->d_dir, dir.data(), sizeof(int) * dir.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fpm_fail(h, FMD_ERR_DEVICE, "copy failed");
    }
    std::vector<int> st((size_t)n_tracks + 1, 0);
    for (int t = 0; t <= n_tracks && n_tracks > 0; t++) st[(size_t)t] = (int)starts[t];
    if (D > 0 && hipMemcpy(h->d_cat, words, sizeof(uint32_t) * (size_t)D, hipMemcpyHostToDevice) != hipSuccess) return fpm_fail(h, FMD_ERR_DEVICE, "copy failed");
    if (hipMemcpy(h->d_starts, st.data(), sizeof(int) * st.size(), hipMemcpyHostToDevice) != hipSuccess) return fpm_fail(h, FMD_ERR_DEVICE, "copy failed");
    h->D = (int)D;
    h->T = n_tracks;
    const long long most = D > h->cfg.n_channels ? D : h->cfg.n_channels;
    hipLaunchKernelGGL(k_fpmatch_loaded, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, nullptr, h->cfg.n_channels, h->d_status, h->d_cat, (int)D, h->lay.mask);
    if (const char* e = fmd::control_end("k_fpmatch_loaded launch failed")) return fpm_fail(h, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_fpmatch_process_dev(fmd_fpmatch h, const uint32_t* d_words, long long words_stride, const int* d_nwords, int n, const uint8_t* d_active,
                            fmd_fpmatch_event* d_events, long long events_stride, int* d_nevents, uint8_t* d_flags, uint8_t* d_ok, void* stream) {
    if (!h) return FMD_ERR_ARG;
    if (!d_words || reinterpret_cast<uintptr_t>(d_words) % 4 != 0) return fpm_fail(h, FMD_ERR_ARG, "null words, or words not aligned to 4 bytes");
    if (!d_events || reinterpret_cast<uintptr_t>(d_events) % 8 != 0) return fpm_fail(h, FMD_ERR_ARG, "null events, or events not aligned to 8 bytes");
    if (reinterpret_cast<uintptr_t>(d_nwords) % 4 != 0 || reinterpret_cast<uintptr_t>(d_nevents) % 4 != 0) return fpm_fail(h, FMD_ERR_ARG, "counts not aligned to 4 bytes");
    if (n < 0 || n > words_stride || n > h->cfg.max_words)
        return fpm_fail(h, FMD_ERR_ARG, "n %d outside [0, words_stride %lld] or above max_words %d", n, words_stride, h->cfg.max_words);
    const long long need = fmd_fpmatch_max_events(h->cfg.interval, n);
    if (events_stride < need) return fpm_fail(h, FMD_ERR_ARG, "events_stride %lld below the %lld events the call may write", events_stride, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const char* e = h->order.begin(s)) return fpm_fail(h, FMD_ERR_DEVICE, "%s", e);
    const int C = h->cfg.n_channels, W = h->cfg.block;
    const long long rows_max = (long long)C * need;                          // the host never learns the count: launched for the most
    const long long tiles = fmd::fpmatch_tiles(h->D, W);
    const int G = (int)(tiles < h->lay.groups ? tiles : h->lay.groups);      // 0 with an empty catalogue
    hipLaunchKernelGGL(k_fpmatch_map, dim3(1), dim3(fmd::rowmap::kThreads), 0, s, h->dev, n, d_nwords, d_active, h->d_status, h->d_qbase);
    // the two objects' launch conditions are not one: a catalogue shorter than a window (D > 0, G = 0) is probed and is not searched
    const bool searched = !h->indexed && rows_max > 0 && G > 0;
    const bool probed = h->indexed && rows_max > 0 && h->D > 0;
    if (searched || probed)
        hipLaunchKernelGGL(k_fpmatch_gather, dim3((unsigned)rows_max), dim3(64), 0, s, h->dev, n, d_nwords, h->d_status, h->d_qbase, h->d_ring, d_words, words_stride,
                           h->d_qwin);
    if (h->indexed) {
        if (probed) {
            const FpmIdxDev x{h->d_keys, h->d_pos, h->d_dir, h->ilay.dir_bits, h->icfg.max_bucket, h->ilay.chunk_words, h->icfg.follow};
            hipLaunchKernelGGL(k_fpmatch_probe, dim3((unsigned)rows_max), dim3(kFpmIndexThreads), 0, s, C, W, h->d_qbase, h->d_qwin, h->d_cat, h->D, h->d_starts, h->T, x,
                               h->d_part, h->d_rowstat);
        }
        hipLaunchKernelGGL(k_fpmatch_finish_idx, dim3((unsigned)C), dim3(64), 0, s, h->dev, n, d_nwords, d_active, h->d_qbase, h->d_part, h->d_rowstat, probed ? 1 : 0,
                           h->d_qwin, h->d_cat, h->D, h->icfg.follow, h->d_starts, h->T, d_words, words_stride, h->d_status, h->d_istatus, h->d_ring, d_events,
                           events_stride, d_nevents, d_flags, d_ok);
    } else {
        if (searched)
            hipLaunchKernelGGL(k_fpmatch_search, dim3((unsigned)((rows_max + kQR - 1) / kQR), (unsigned)G), dim3(kFpmatchThreads), sizeof(uint32_t) * (size_t)h->lay.lds_words,
                               s, C, W, h->d_qbase, h->d_qwin, h->d_cat, h->D, h->d_starts, h->T, G, h->d_part);
        hipLaunchKernelGGL(k_fpmatch_finish, dim3((unsigned)C), dim3(64), 0, s, h->dev, n, d_nwords, d_active, h->d_qbase, h->d_part, G, h->d_starts, h->T, d_words,
                           words_stride, h->d_status, h->d_ring, d_events, events_stride, d_nevents, d_flags, d_ok);
    }
    if (hipGetLastError() != hipSuccess) return fpm_fail(h, FMD_ERR_DEVICE, "k_fpmatch launch failed");
    if (const char* e = h->order.end(s)) return fpm_fail(h, FMD_ERR_DEVICE, "%s", e);
    return FMD_OK;
}

int fmd_fpmatch_get_status(fmd_fpmatch h, fmd_fpmatch_status* out) {
    if (!h || !out) return fpm_fail(h, FMD_ERR_ARG, "null object or output");
    if (!h->order.quiesce()) return fpm_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, h->d_status, sizeof(fmd_fpmatch_status) * (size_t)h->cfg.n_channels, hipMemcpyDeviceToHost) != hipSuccess)
        return fpm_fail(h, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

int fmd_fpmatch_status_dev(fmd_fpmatch h, const fmd_fpmatch_status** d_status) {
    if (!h || !d_status) return fpm_fail(h, FMD_ERR_ARG, "null object or output");
    *d_status = h->d_status;
    return FMD_OK;
}

int fmd_fpmatch_get_index_status(fmd_fpmatch h, fmd_fpmatch_index_status* out) {
    if (!h || !out) return fpm_fail(h, FMD_ERR_ARG, "null object or output");
    if (!h->indexed) return fpm_fail(h, FMD_ERR_STATE, "the object was created without an index");
    if (!h->order.quiesce()) return fpm_fail(h, FMD_ERR_DEVICE, "synchronise failed");
    if (hipMemcpy(out, h->d_istatus, sizeof(fmd_fpmatch_index_status) * (size_t)h->cfg.n_channels, hipMemcpyDeviceToHost) != hipSuccess)
        return fpm_fail(h, FMD_ERR_DEVICE, "copy failed");
    return FMD_OK;
}

const char* fmd_fpmatch_last_error(fmd_fpmatch h) { return h ? h->err.c_str() : fmd::fpmatch_global_error().c_str(); }

}  // extern "C"
