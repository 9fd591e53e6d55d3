// Which kernels a handle's blocks get, and with which launch geometry.  Host only (no HIP include: tests/cpp/plan_main.cpp builds it with
// plain g++).  Two levels:
//   Plan       what the batch size decides: every station-count threshold of the demodulator and the rules that combine them.  fmd_create makes
//              one per handle (fmd_debug_pll_adaptive replaces it); fmd_debug_plan (include/fmdemod_debug.h) shows it to the tests.
//   BlockPlan  what the block length, the input type and the run-time facts (PlanFacts: what the controls and the debug hooks have set) decide on
//              top of it: each stage's kernel form, tile, workgroup count and name.  refresh_block_plan (fmd_kernels.h) makes it whenever a fact
//              can have changed; fmd_debug_block_plan shows it to the tests.
// The stage launchers of fmd_kernels.hip decide nothing: they turn these fields into template parameters and grids.  The one decision made per
// block is pll_kernel().
#pragma once

#include <climits>
#include <cstddef>

#include "fmdemod.h"

namespace fmd {

// Batch size the latency/throughput switches are keyed on: the stages behind the first decimator cost the same at every input
// rate; the decimator itself (m > 1) adds FIR work and HBM traffic that compete with the serial kernels (measured cross-overs: x 1.5).
inline int effective_channels(int C, int m) { return m == 1 ? C : C + C / 2; }

// Thresholds named ...Eff compare with effective_channels(), ...Stations with the raw station count.

// Which pilot-PLL kernel: the time-parallel one halves a lone wavefront's latency for 2.6x the VALU work.  Once the chip's
// VALU throughput bounds the step the low-work kernel is faster (measured cross-over: between 7168 and 8192 channels at
// 256 kSa/s, about 8192 at 1.024 MSa/s).
constexpr int kPllTimeParallelMaxStations = 7168;
// within the time-parallel kernel: 16 lanes per channel while a lone wavefront's latency is what matters (same-box A/B:
// 8 % faster at 2560 channels, 6 % at 3072), 8 lanes per channel (30 % fewer VALU instructions) beyond (2 % faster at 4096)
constexpr int kPllK16MaxEff = 3584;
// (two ranges: 3585 .. 4096 effective stations — 8 or 16 lanes of the time-parallel kernel; above kPllTimeParallelMaxStations, up to 16384 stations —
//  the low-work kernel or the time-parallel one with 8 lanes, whose sequence form gets through loops out of lock: 8192 stations with 1 % unlocked
//  2.87 -> 1.9 ms a block.  The FMD_FLAG_PLL_* selectors switch the choice off.)
constexpr int kPllK16UnlockedMaxEff = 4096;          // 16 lanes while wavefronts are out of lock, up to here
constexpr int kPllAdaptiveMaxStations = 16384;       // the low-work kernel gives way to the time-parallel one out of lock, up to here
// per-wavefront hand-over between consecutive k_pilot_pll launches: the time-parallel kernel only, pipelined mode only, up to here (the
// measurements: the comment at the hand-over in k_pilot_pll, fmd_kernels.hip)
constexpr int kPllChainMaxEff = 3328;
// k_pilot_power<true>: the batches whose step is this kernel's latency (and whose PLL launches hand over per wavefront)
constexpr int kPowerRowsMaxEff = 2816;
constexpr int kLmrInlineMax = 512;   // estimates per block (n_audio / 10) up to which k_extract integrates the L-R phase itself
// Tolerance mode, batches up to 6144 stations: same-box A/B +3 % at 4096 stations, but -3 % at 8192 and -4 % at 16384 (there the
// k_extract launches running back to back crowd k_front out: its launches take 1.7x as long); and in the exact mode the pilot
// PLL's launch chain sets the step, which k_extract launches without gaps between them slow down (-8 %).
constexpr int kLmrInlineMaxEff = 6144;
// fmd_submit_* puts a block's extract stage off until the next block's front end is queued (launch_deferred) from 1024 stations'
// worth of 256 kSa/s blocks on (same-box A/B with the three-wavefront RDS stage: +-0 at 1024 stations, +1 % at 1536, +6 % at 2048,
// +10 % at 2560, +6-7 % from 3072 on; smaller batches are pure stage latency and keep every stage on a queue of its own)
constexpr size_t kLazyMinSamples = (size_t)1024 * 8192;          // stations x fm_out samples of a block
// Batches of 1024 .. 1792 stations at 256 kSa/s (the smallest on the deferred schedule — kLazyMinSamples — up to where the front end's own length takes over): the serial RDS stage's launch is the step (0.092 ms alone, 0.12 beside the throughput kernels)
// and the front end has slack.  With 44 KB of extra dynamic LDS its workgroups come two to a CU instead of six and leave the serial stages'
// wavefronts the issue slots: 1024 stations 0.125 -> 0.114 ms (RDS launch 0.121 -> 0.102, the front end itself 0.060 -> 0.053), 1536 stations
// 0.135 -> 0.126, 1792: 0.144 -> 0.136, 1024 x u8 0.117 -> 0.110; 512 stations and the 40 of configs[4]: no difference; 640: slower (0.111 ->
// 0.120: no deferred schedule there), 2048: slower (0.148 -> 0.154) (profiles/round5/rds_stage_ab.txt).
constexpr int kFrontPadMinStations = 1024, kFrontPadMaxStations = 1792, kFrontPadBytes = 45056;
inline int front_lds_pad(int C, int m) { return (m == 1 && C >= kFrontPadMinStations && C <= kFrontPadMaxStations) ? kFrontPadBytes : 0; }
// cf32 captures, round 6: 2048-output tiles for batches that still give the chip 12 288 workgroups (3072 stations' worth of 64 ms blocks) —
// half as many workgroups fetch the FIR's operand images (7 KB each from L2: 230 MB a block at 1024-output tiles) and recompute a
// tile's 63-sample halo: k_front_mfma 0.154 -> 0.142 ms in the step, 268 -> 278 GSa/s at 4096 stations, +2.5 % at 8192; at 2048 stations
// (8192 workgroups) 1024-output tiles are 1 % better (profiles/round6/front_tile_ab.txt).
constexpr long kFrontBigTileMinWorkgroups = 12288;
// k_extract_bp: the workgroups the chip wants (4 per CU: a round and a half) — what make_block_plan's tile search leaves, and what the
// station pairs of k_extract_bp<2> must still be
constexpr int kExtractMinWorkgroups = 1536;

// Up to which batch the pilot PLL runs as the time-parallel kernel at all (raw stations) and with 16 lanes a station (effective stations)
struct PllThresholds { int k16_max; int time_parallel_max; };
inline PllThresholds default_pll_thresholds(unsigned flags) {
    return {(flags & FMD_FLAG_PLL_K8) ? 0 : kPllK16MaxEff,
            (flags & FMD_FLAG_PLL_LOW_WORK) ? 0 : ((flags & FMD_FLAG_PLL_TIME_PARALLEL) ? INT_MAX : kPllTimeParallelMaxStations)};
}

struct Plan {
    int channels, effective;     // the station count and effective_channels() of it
    int m, n_fm_in, n_fm_out, n_audio, n_est;   // the block: first decimation (1, 4, 8) and its lengths along the pipeline (fmd_kernels.h Dims)
    bool fast, keep_taps;        // FMD_FLAG_FAST_MATH, FMD_FLAG_KEEP_TAPS
    PllThresholds pll;           // in force: default_pll_thresholds(), or what fmd_debug_pll_adaptive moved them to
    bool power_rows;             // k_pilot_power<true>, not <false>
    bool pll_k_adaptive;         // exact mode: the pilot-PLL kernel follows what is out of lock, block by block (pll_kernel())
    bool pll_chained;            // consecutive k_pilot_pll launches hand over per wavefront
    int pll_waves;               // wavefronts the hand-over array Buffers::pll_chain is allocated for
    bool lmr_inline;             // k_extract integrates the previous block's L-R phase estimates itself (no k_lmr_phase launch)
    bool lazy_capable;           // fmd_submit_*: a block's extract stage waits for the next block's front end
    int front_lds_pad;           // bytes of dynamic LDS k_front_mfma asks for beyond its need
    bool front_big_tile;         // cf32 captures: 2048-output front-end tiles where the block length allows
    bool extract_auto_pair;      // k_extract_bp<2> where make_block_plan's other conditions hold
};

// moved: fmd_debug_pll_adaptive's thresholds (exact mode, up to kPllK16UnlockedMaxEff effective stations: the caller checks).  The hook keeps its
// own, shorter rule: adaptive whenever a threshold lies below the batch, whatever the FMD_FLAG_PLL_* selectors say; never chained (the per-wavefront
// hand-over is indexed by wavefront: one kernel, one lane count only); and pll_waves stays what the default thresholds give, since the array it
// sizes was allocated when the handle was created.
Plan make_plan(int C, int m, int n_fm_out, int n_est, unsigned flags, const PllThresholds* moved = nullptr);

enum class PllKernel : int { LowWork = 0, TimeParallel16 = 1, TimeParallel8 = 2 };
// The one per-block decision, exact mode: unlocked_now = wavefronts ran out of lock in the last blocks the host has seen (fmd_api.cpp) — the
// low-work kernel gives way to the time-parallel one, whose sequence form gets through such loops; the time-parallel kernel takes 16 lanes a
// station up to kPllK16UnlockedMaxEff
PllKernel pll_kernel(const Plan& p, bool unlocked_now);

// What the controls (fmd_api.cpp upload_controls) and the debug hooks leave behind, between blocks
struct PlanFacts {
    bool any_deemph = false;        // a station's de-emphasis runs as a stage of its own (k_deemphasis)
    bool deemph_in_tile = false;    // FMD_FLAG_FAST_MATH: the de-emphasis IIR runs inside k_front_mfma's tile (every filtering station's pole <= 0.905, i.e. up to ~79 us)
    bool split_front = false;       // fmd_debug_split_front: 1.024 / 2.048 MSa/s tolerance mode with k_predecim_mfma and k_front_mfma as two kernels (the parity check of k_front_pre_mfma)
    bool uniform_cutoffs = false;   // every station has the same L+R / L-R cut-offs: one set of k_extract_bp's tap tables serves any of them
    int extract_pairing = 0;        // k_extract_bp with two stations per workgroup: 0 = where it pays (Plan::extract_auto_pair), 1 = wherever possible (tests), 2 = never
};

// fmd_create only admits blocks of 1024 m samples, so n_fm_out is a multiple of 512 and n_audio = n_fm_out / 4 one of 128: "the block is a whole
// number of 1024-output front tiles" and "of 256-sample extract tiles" are one fact
inline bool whole_tiles(const Plan& p) { return p.n_fm_out % 1024 == 0; }

// Tolerance mode at 1.024 / 2.048 MSa/s (m > 1): the first decimator runs inside the front end's kernel (k_front_pre_mfma) and the block has no
// decimator stage of its own, unless a de-emphasis filter is on (as a stage or in k_front's tile), the block length does not fit the tiles, or
// fmd_debug_split_front asks for the two kernels.  make_block_plan and the schedule (fmd_schedule.cpp) both ask.
inline bool front_takes_capture(const Plan& p, const PlanFacts& f) {
    return p.m > 1 && p.fast && !f.any_deemph && !f.deemph_in_tile && whole_tiles(p) && !f.split_front;
}

// The stages of one block (the schedule places them on queues, fmd_schedule.h) and the names fmd_profile_read reports them under: the exact mode's
// kernels and the tolerance mode's, as they appear in rocprofv3 kernel traces
enum Stage { ST_FRONT = 0, ST_DEEMPH, ST_POWER, ST_PLL, ST_EXTRACT, ST_RDS, ST_PREDECIM, ST_COUNT };
extern const char* const kStageName[ST_COUNT];
extern const char* const kStageNameFast[ST_COUNT];

constexpr int kFrontDeemphWarmup = 128;   // fm_out samples k_front_mfma's in-tile de-emphasis starts early (fmd_kernels.hip kDeemphWarmup)
constexpr int kExtractNtMax = 0x7fff;     // k_extract_bp: tiles per wavefront travel in the low 16 bits of one kernel argument (bit 16: a development switch)

enum class FrontKernel : int { Front = 0, FrontMfma = 1, FrontPreMfma = 2 };                 // k_front, k_front_mfma, k_front_pre_mfma
// what the front end reads: the capture, or behind a first-decimator stage fm_in as samples (exact mode) or as their phases in turns (k_predecim_mfma)
enum class FrontInput : int { Cf32 = 0, U8 = 1, FmIn = 2, Phases = 3 };
enum class PredecimKernel : int { None = 0, Plain = 1, Phases = 2, Mfma = 3 };               // no stage, k_predecim<.., false>, k_predecim<.., true>, k_predecim_mfma
enum class LmrPhase : int { Inline = 0, Fast = 1, Serial = 2 };                              // inside the extract kernel, k_lmr_phase_fast, k_lmr_phase
enum class RdsKernel : int { Sync = 0, SyncFast = 1, Sync3 = 2 };                            // k_rds_sync<false>, k_rds_sync<true>, k_rds_sync3

struct BlockPlan {
    bool iq_streams;             // the handle materialises fm_out_iq / pll_dt: everything but the tolerance mode without FMD_FLAG_KEEP_TAPS on blocks of whole 256-sample extract tiles
    // front end
    FrontKernel front;
    int front_warmup;            // k_front_mfma: 0 or kFrontDeemphWarmup (the de-emphasis IIR inside the tile)
    int front_lds_pad;           // bytes of dynamic LDS k_front_mfma asks for beyond its need: by the station count alone, it always sees a 256 kSa/s stream
    // the two stages that read the capture, per input type ([0] cf32, [1] u8).  Workgroup counts: stations x tiles, without the fused pilot workgroups
    struct Input {
        FrontInput front_input;
        int front_tile, front_workgroups;         // fm_out samples per workgroup: 512, 1024 or 2048
        PredecimKernel predecim;                  // None exactly when the front end takes the capture (m == 1, or front == FrontPreMfma)
        int predecim_tile, predecim_workgroups;   // fm_in samples per workgroup
    } in[2];
    // de-emphasis stage: k_deemphasis + k_pilot_sums on the plane (tolerance mode) or k_deemphasis + k_hilbert
    bool deemph_pilot_sums;
    int deemph_workgroups;       // of the second kernel of the pair
    LmrPhase lmr_phase;          // the extract launcher and the "lmr_phase" getter's peek both go by it (the peek: k_lmr_phase_fast unless Serial)
    // extract stage
    int extract_tile;            // audio samples: 128 or 256
    bool extract_bp;             // k_extract_bp, not k_extract
    int extract_nt;              // k_extract_bp: tiles per wavefront, 1 .. kExtractNtMax
    bool extract_pair;           // k_extract_bp<2>: two stations per workgroup
    int extract_grid_x;
    RdsKernel rds;
    int rds_partials;            // partial sums of |rds|^2 per station the kernel is told of (k_extract_bp leaves them for k_rds_sync3)
    const char* stage_name[ST_COUNT];
};
BlockPlan make_block_plan(const Plan& p, const PlanFacts& f);

}  // namespace fmd
