// The rules of fmd_plan.h.  Host only.
#include "fmd_plan.h"

#include "fmd_tables.h"

namespace fmd {

Plan make_plan(int C, int m, int n_fm_out, int n_est, unsigned flags, const PllThresholds* moved) {
    const bool fast = (flags & FMD_FLAG_FAST_MATH) != 0, pipelined = (flags & FMD_FLAG_NO_PIPELINE) == 0, keep_taps = (flags & FMD_FLAG_KEEP_TAPS) != 0;
    Plan p{};
    p.m = m; p.n_fm_in = 2 * n_fm_out; p.n_fm_out = n_fm_out; p.n_audio = n_fm_out / 4; p.n_est = n_est;
    p.fast = fast; p.keep_taps = keep_taps;
    p.channels = C;
    p.effective = effective_channels(C, m);
    p.pll = default_pll_thresholds(flags);
    // the raw station count, where every neighbouring switch takes the effective one: as measured (kPllTimeParallelMaxStations)
    const bool time_parallel = C <= p.pll.time_parallel_max;
    p.pll_k_adaptive = !fast &&
                       ((time_parallel && !(flags & (FMD_FLAG_PLL_K8 | FMD_FLAG_PLL_LOW_WORK)) && p.effective > p.pll.k16_max && p.effective <= kPllK16UnlockedMaxEff) ||
                        (!time_parallel && !(flags & FMD_FLAG_PLL_LOW_WORK) && C <= kPllAdaptiveMaxStations));
    // (the low-work kernel k_pilot_pll_pairs has no chain argument: its launches must stay ordered by the stream)
    // (FMD_FLAG_KEEP_TAPS: k_pll_taps reads the loop's start state ahead of the PLL kernel — consecutive blocks' launches stay in stream order;
    //  the hand-over is indexed by wavefront, so it never runs beside the adaptive lane count)
    p.pll_chained = pipelined && !fast && !keep_taps && time_parallel && p.effective <= kPllChainMaxEff && !(flags & (FMD_FLAG_PLL_STREAM_ORDER | FMD_FLAG_PLL_LOW_WORK)) &&
                    !p.pll_k_adaptive;
    // a wavefront of k_pilot_pll<16> holds 4 stations, one of k_pilot_pll<8> holds 8: whichever of pll_kernel()'s answers has more wavefronts
    p.pll_waves = (p.effective <= p.pll.k16_max || (p.pll_k_adaptive && time_parallel)) ? (C + 3) / 4 : (C + 7) / 8;
    if (moved) {
        p.pll = *moved;
        p.pll_k_adaptive = C > moved->time_parallel_max || p.effective > moved->k16_max;
        p.pll_chained = false;
    }
    p.power_rows = p.effective <= kPowerRowsMaxEff;
    p.lmr_inline = fast && n_est <= kLmrInlineMax && p.effective <= kLmrInlineMaxEff;
    p.lazy_capable = pipelined && fast && (size_t)C * n_fm_out >= kLazyMinSamples;
    p.front_lds_pad = front_lds_pad(C, m);
    p.front_big_tile = (long)C * (n_fm_out / 2048) >= kFrontBigTileMinWorkgroups;
    p.extract_auto_pair = (C + 1) / 2 >= kExtractMinWorkgroups;
    return p;
}

PllKernel pll_kernel(const Plan& p, bool unlocked_now) {
    if (p.channels > p.pll.time_parallel_max && !unlocked_now) return PllKernel::LowWork;
    if (p.effective <= p.pll.k16_max || (unlocked_now && p.effective <= kPllK16UnlockedMaxEff)) return PllKernel::TimeParallel16;
    return PllKernel::TimeParallel8;
}

const char* const kStageName[ST_COUNT] = {"k_front", "k_deemphasis+k_hilbert", "k_pilot_power", "k_pilot_pll", "k_extract", "k_rds_sync", "k_predecim"};
const char* const kStageNameFast[ST_COUNT] = {"k_front_mfma", "k_deemphasis", "k_pilot_power", "k_pll_sparse", "k_extract_bp", "k_rds_sync", "k_predecim_mfma"};

namespace {

// k_front / k_front_mfma: 1024 outputs a workgroup whenever the block allows it (fmd_kernels.hip FrontGeom); 2048 in the tolerance mode without
// in-tile de-emphasis, for u8 captures always (4 KB of input per 1024-output workgroup leaves too few bytes in flight per CU), for cf32 captures in
// the batches of Plan::front_big_tile, behind the first decimator never
int front_tile(const Plan& p, const PlanFacts& f, FrontInput in) {
    const bool big = p.fast && p.n_fm_out % 2048 == 0 && !f.deemph_in_tile && (in == FrontInput::U8 || (in == FrontInput::Cf32 && p.front_big_tile));
    return big ? 2048 : (whole_tiles(p) ? 1024 : 512);
}

// k_extract_bp: a workgroup = station x 4 nt tiles, nt per wavefront (the station's tap tables are staged once per workgroup): the largest nt that
// still leaves kExtractMinWorkgroups for the chip.  Two stations per workgroup (tables and the block edge's matrix fetched once for both) where a
// station is one workgroup anyway, every station has the same cut-offs and the pairs still are kExtractMinWorkgroups (Plan::extract_auto_pair)
void extract_bp_geometry(const Plan& p, const PlanFacts& f, BlockPlan& b) {
    const int tiles = p.n_audio / 256, C = p.channels;
    int nt = 1;
    // (block_size has no cap, so the search is clamped: at 8 bits a block of a million samples could wrap nt to 0)
    for (int v = (tiles + 3) / 4 < kExtractNtMax ? (tiles + 3) / 4 : kExtractNtMax; v >= 1; v--)
        if ((long)((tiles + 4 * v - 1) / (4 * v)) * C >= kExtractMinWorkgroups) { nt = v; break; }
    const bool one_wg_per_station = 4 * nt >= tiles;
    b.extract_pair = f.uniform_cutoffs && one_wg_per_station && 2 * tiles <= 4 * kExtractNtMax && C >= 2 &&
                     (f.extract_pairing == 1 || (f.extract_pairing == 0 && p.extract_auto_pair));
    b.extract_nt = b.extract_pair ? (2 * tiles + 3) / 4 : nt;
    b.extract_grid_x = b.extract_pair ? (C + 1) / 2 : (tiles + 4 * nt - 1) / (4 * nt) * C;
}

}  // namespace

BlockPlan make_block_plan(const Plan& p, const PlanFacts& f) {
    const int C = p.channels;
    BlockPlan b{};
    b.iq_streams = !p.fast || p.keep_taps || !whole_tiles(p);
    const bool pre = front_takes_capture(p, f);
    b.front = pre ? FrontKernel::FrontPreMfma : (p.fast ? FrontKernel::FrontMfma : FrontKernel::Front);
    b.front_warmup = (b.front == FrontKernel::FrontMfma && f.deemph_in_tile) ? kFrontDeemphWarmup : 0;
    b.front_lds_pad = b.front == FrontKernel::FrontMfma ? front_lds_pad(C, 1) : 0;
    for (int u8 = 0; u8 < 2; u8++) {
        BlockPlan::Input& in = b.in[u8];
        const bool stage = p.m > 1 && !pre;       // the first decimator as a stage of its own
        in.front_input = stage ? (p.fast ? FrontInput::Phases : FrontInput::FmIn) : (u8 ? FrontInput::U8 : FrontInput::Cf32);
        in.front_tile = pre ? 1024 : front_tile(p, f, in.front_input);
        in.front_workgroups = p.n_fm_out / in.front_tile * C;
        if (!stage) continue;                     // (PredecimKernel::None, no tile)
        // k_predecim_mfma's tile: 2048 input samples of cf32 (16 KB; the kernel then sits on its HBM floor whatever the tile), 8192 of u8 (16 KB as
        // well: with 4 KB per workgroup too few bytes are in flight per CU); blocks that are no multiple of it: 256 outputs per workgroup
        const int full = (u8 ? 8192 : 2048) / p.m;
        if (p.fast && p.n_fm_in % full == 0) { in.predecim = PredecimKernel::Mfma; in.predecim_tile = full; }
        else if (p.fast && p.n_fm_in % 256 == 0) { in.predecim = PredecimKernel::Mfma; in.predecim_tile = 256; }
        else { in.predecim = p.fast ? PredecimKernel::Phases : PredecimKernel::Plain; in.predecim_tile = 512; }      // (fmd_kernels.hip PredecimGeom::TP)
        in.predecim_workgroups = p.n_fm_in / in.predecim_tile * C;
    }
    b.deemph_pilot_sums = p.fast;
    b.deemph_workgroups = p.fast ? C * ((p.n_fm_out / kSparseDec + 63) / 64) : p.n_fm_out / 256 * C;
    // k_lmr_phase_fast takes blocks of up to kLmrInlineMax estimates, like the inline form (which Plan::lmr_inline also keeps to the smaller batches)
    b.lmr_phase = p.lmr_inline ? LmrPhase::Inline : ((p.fast && p.n_est <= kLmrInlineMax) ? LmrPhase::Fast : LmrPhase::Serial);
    b.extract_tile = whole_tiles(p) ? 256 : 128;
    b.extract_bp = p.fast && whole_tiles(p);
    if (b.extract_bp) extract_bp_geometry(p, f, b);
    else b.extract_grid_x = p.n_audio / b.extract_tile * C;
    // k_rds_sync3 where k_extract_bp ran and left the block's power as 2 partial sums per tile
    b.rds = !p.fast ? RdsKernel::Sync : (b.extract_bp ? RdsKernel::Sync3 : RdsKernel::SyncFast);
    b.rds_partials = p.fast ? 2 * (p.n_audio / 256) : 0;
    for (int i = 0; i < ST_COUNT; i++) b.stage_name[i] = (p.fast ? kStageNameFast : kStageName)[i];      // (the tolerance mode's extract stage: under this name with either kernel)
    if (pre) b.stage_name[ST_FRONT] = "k_front_pre_mfma";
    return b;
}

}  // namespace fmd
