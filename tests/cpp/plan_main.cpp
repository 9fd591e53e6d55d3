// fm-radio_amd/csrc/fmd_plan.cpp on its own (no HIP, no library): built with -fsanitize=address,undefined by `make -C oracle asan`.
// Reads configurations, one a line: C m n_fm_out n_est flags k16_max time_parallel_max unlocked_now (thresholds < 0: the defaults),
// and prints the plan's fields in the order of include/fmdemod_debug.h's fmd_plan_info.  With a second file, one block-plan case a line:
// C m n_fm_out n_est flags u8 any_deemph deemph_in_tile split_front uniform_cutoffs extract_pairing, it then prints "--" and the block plan's
// fields in the order of fmd_block_plan_info.  tests/test_sanitizers_cpu.py compares both with tests/plan_model.py.
#include <cstdio>

#include "fmd_plan.h"

int main(int argc, char** argv) {
    if (argc != 2 && argc != 3) { std::fprintf(stderr, "usage: plan_main cases.txt [block_cases.txt]\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    int C, m, n_fm_out, n_est, k16, tp, unlocked;
    unsigned flags;
    long n = 0;
    while (std::fscanf(f, "%d %d %d %d %u %d %d %d", &C, &m, &n_fm_out, &n_est, &flags, &k16, &tp, &unlocked) == 8) {
        const fmd::PllThresholds moved{k16, tp};
        const fmd::Plan p = fmd::make_plan(C, m, n_fm_out, n_est, flags, k16 >= 0 ? &moved : nullptr);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d\n", p.effective, (int)p.power_rows, (int)p.pll_k_adaptive, (int)p.pll_chained, p.pll_waves, (int)p.lmr_inline,
                    (int)p.lazy_capable, p.front_lds_pad, (int)p.front_big_tile, (int)p.extract_auto_pair, (int)fmd::pll_kernel(p, unlocked != 0));
        n++;
    }
    std::fclose(f);
    if (argc == 3) {
        if (!(f = std::fopen(argv[2], "r"))) { std::perror(argv[2]); return 2; }
        std::printf("--\n");
        int u8, any_deemph, in_tile, split, uniform, pairing;
        while (std::fscanf(f, "%d %d %d %d %u %d %d %d %d %d %d", &C, &m, &n_fm_out, &n_est, &flags, &u8, &any_deemph, &in_tile, &split, &uniform, &pairing) == 11) {
            const fmd::Plan p = fmd::make_plan(C, m, n_fm_out, n_est, flags);
            fmd::PlanFacts facts;
            facts.any_deemph = any_deemph != 0; facts.deemph_in_tile = in_tile != 0; facts.split_front = split != 0; facts.uniform_cutoffs = uniform != 0;
            facts.extract_pairing = pairing;
            const fmd::BlockPlan b = fmd::make_block_plan(p, facts);
            const fmd::BlockPlan::Input& in = b.in[u8 != 0];
            std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s %s\n", (int)b.iq_streams, (int)b.front, (int)in.front_input, in.front_tile, b.front_warmup,
                        in.front_workgroups, b.front_lds_pad, (int)in.predecim, in.predecim_tile, in.predecim_workgroups, (int)b.deemph_pilot_sums, b.deemph_workgroups,
                        (int)p.power_rows, (int)b.lmr_phase, b.extract_tile, (int)b.extract_bp, b.extract_nt, (int)b.extract_pair, b.extract_grid_x, (int)b.rds, b.rds_partials,
                        b.stage_name[fmd::ST_FRONT], b.stage_name[fmd::ST_EXTRACT]);
            n++;
        }
        std::fclose(f);
    }
    return n > 0 ? 0 : 1;
}
