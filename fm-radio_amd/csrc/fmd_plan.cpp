// The rules of fmd_plan.h.  Host only.
#include "fmd_plan.h"

namespace fmd {

Plan make_plan(int C, int m, int n_fm_out, int n_est, unsigned flags, const PllThresholds* moved) {
    const bool fast = (flags & FMD_FLAG_FAST_MATH) != 0, pipelined = (flags & FMD_FLAG_NO_PIPELINE) == 0, keep_taps = (flags & FMD_FLAG_KEEP_TAPS) != 0;
    Plan p{};
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

}  // namespace fmd
