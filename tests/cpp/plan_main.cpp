// fm-radio_amd/csrc/fmd_plan.cpp on its own (no HIP, no library): built with -fsanitize=address,undefined by `make -C oracle asan`.
// Reads configurations, one a line: C m n_fm_out n_est flags k16_max time_parallel_max unlocked_now (thresholds < 0: the defaults),
// and prints the plan's fields in the order of include/fmdemod_debug.h's fmd_plan_info.  tests/test_sanitizers_cpu.py compares them with
// tests/plan_model.py.
#include <cstdio>

#include "fmd_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: plan_main cases.txt\n"); return 2; }
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
    return n > 0 ? 0 : 1;
}
