"""Which kernels the library picks for a configuration, restated in Python from the rules as fmd_create, fmd_debug_pll_adaptive and the stage
launchers spelled them out before fm-radio_amd/csrc/fmd_plan.h gathered them (bare numbers on purpose: this is the independent side of
tests/test_plan_cpu.py and of the sanitizer run of tests/cpp/plan_main.cpp, and shares no constant with the library)."""
KEEP_TAPS, NO_PIPELINE, PLL_TIME_PARALLEL, PLL_LOW_WORK, PLL_K8, PLL_STREAM_ORDER, FAST_MATH = 1, 2, 4, 8, 16, 32, 64
LOW_WORK, TIME_PARALLEL_16, TIME_PARALLEL_8 = 0, 1, 2
FIELDS = ("effective_channels", "pilot_power_rows", "pll_k_adaptive", "pll_chained", "pll_waves", "lmr_inline", "lazy_capable", "front_lds_pad",
          "front_big_tile", "extract_auto_pair", "pll_kernel")


def lengths(fs: int, block_size: int):
    """(m, n_fm_out, n_est) of a block."""
    m = fs // 256_000
    n_fm_out = block_size // m // 2
    return m, n_fm_out, (n_fm_out // 4 + 9) // 10


def plan(C: int, m: int, n_fm_out: int, n_est: int, flags: int, thresholds=None, unlocked_now: bool = False) -> tuple:
    """The values of FIELDS.  thresholds = (k16_max, time_parallel_max): what fmd_debug_pll_adaptive leaves behind."""
    fast, pipelined, keep_taps = bool(flags & FAST_MATH), not flags & NO_PIPELINE, bool(flags & KEEP_TAPS)
    eff = C if m == 1 else C + C // 2
    tp_max = 0 if flags & PLL_LOW_WORK else (0x7fffffff if flags & PLL_TIME_PARALLEL else 7168)
    k16_max = 0 if flags & PLL_K8 else 3584
    time_parallel = C <= tp_max                      # the station count itself, not eff
    k_adaptive = not fast and ((time_parallel and not flags & (PLL_K8 | PLL_LOW_WORK) and k16_max < eff <= 4096) or
                               (not time_parallel and not flags & PLL_LOW_WORK and C <= 16384))
    chained = (pipelined and not fast and not keep_taps and time_parallel and eff <= 3328 and not flags & (PLL_STREAM_ORDER | PLL_LOW_WORK)
               and not k_adaptive)
    waves = (C + 3) // 4 if eff <= k16_max or (k_adaptive and time_parallel) else (C + 7) // 8
    if thresholds is not None:                       # the hook: its own rule, no hand-over, the array stays as allocated
        k16_max, tp_max = thresholds
        k_adaptive = C > tp_max or eff > k16_max
        chained = False
    if C > tp_max and not unlocked_now:
        kernel = LOW_WORK
    elif eff <= k16_max or (unlocked_now and eff <= 4096):
        kernel = TIME_PARALLEL_16
    else:
        kernel = TIME_PARALLEL_8
    return (eff, int(eff <= 2816), int(k_adaptive), int(chained), waves, int(fast and n_est <= 512 and eff <= 6144),
            int(pipelined and fast and C * n_fm_out >= 1024 * 8192), 45056 if m == 1 and 1024 <= C <= 1792 else 0,
            int(C * (n_fm_out // 2048) >= 12288), int((C + 1) // 2 >= 1536), kernel)


def stations_to_try(step: int = 0) -> list:
    """Station counts within 3 of every switch (those that go by the block length: at 5120, 8192 and 32768 fm_out samples a block), as the station
    count itself and as the count whose effective batch (x 1.5) is there; with step, every step-th count up to 17000 too."""
    marks = (1, 256, 768, 1024, 1639, 1792, 2816, 3072, 3328, 3584, 4096, 6144, 7168, 12288, 16384, 17000 - 3)
    cs = {c for t in marks for base in (t, t * 2 // 3) for c in range(base - 3, base + 4) if c >= 1}
    if step:
        cs.update(range(1, 17001, step))
    return sorted(cs)
