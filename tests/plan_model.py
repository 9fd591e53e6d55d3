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


BLOCK_FIELDS = ("iq_streams", "front_kernel", "front_input", "front_tile", "front_warmup", "front_workgroups", "front_lds_pad", "predecim_kernel", "predecim_tile",
                "predecim_workgroups", "deemph_pilot_sums", "deemph_workgroups", "pilot_power_rows", "lmr_phase", "extract_tile", "extract_bp", "extract_nt",
                "extract_pair", "extract_grid_x", "rds_kernel", "rds_partials")
K_FRONT, K_FRONT_MFMA, K_FRONT_PRE_MFMA = 0, 1, 2
IN_CF32, IN_U8, IN_FM_IN, IN_PHASES = 0, 1, 2, 3
NO_PREDECIM, K_PREDECIM, K_PREDECIM_PHASES, K_PREDECIM_MFMA = 0, 1, 2, 3
LMR_INLINE, LMR_FAST, LMR_SERIAL = 0, 1, 2
K_RDS_SYNC, K_RDS_SYNC_FAST, K_RDS_SYNC3 = 0, 1, 2


def block_plan(C: int, fs: int, block_size: int, flags: int, u8: bool, any_deemph: bool = False, deemph_in_tile: bool = False, split_front: bool = False,
               uniform_cutoffs: bool = False, pairing: int = 0) -> tuple:
    """The values of BLOCK_FIELDS: each stage's kernel form and launch geometry, restated from the stage launchers as they chose them one by one
    (launch_front, launch_predecim, launch_front_pre, launch_stage_front, launch_stage_deemph, launch_extract_ta, launch_stage_extract, launch_stage_rds,
    fmd_create's `streams`) before fm-radio_amd/csrc/fmd_plan.h's BlockPlan gathered them."""
    fast, keep_taps = bool(flags & FAST_MATH), bool(flags & KEEP_TAPS)
    m = fs // 256_000
    n_in = block_size // m
    n_fo = n_in // 2
    n_au = n_fo // 4
    n_est = (n_au + 9) // 10
    eff = C if m == 1 else C + C // 2
    # --- front end: launch_stage_front, launch_front, launch_front_pre
    pre = m > 1 and fast and not any_deemph and not deemph_in_tile and n_fo % 1024 == 0 and not split_front
    if pre:
        kernel, source, tile, warm, pad = K_FRONT_PRE_MFMA, (IN_U8 if u8 else IN_CF32), 1024, 0, 0
    else:
        kernel = K_FRONT_MFMA if fast else K_FRONT
        source = (IN_PHASES if fast else IN_FM_IN) if m > 1 else (IN_U8 if u8 else IN_CF32)
        tile = 512
        if fast and source == IN_CF32 and C * (n_fo // 2048) >= 12288 and n_fo % 2048 == 0 and not deemph_in_tile:
            tile = 2048
        elif fast and source == IN_U8 and n_fo % 2048 == 0 and not deemph_in_tile:
            tile = 2048
        elif n_fo % 1024 == 0:
            tile = 1024
        warm = 128 if fast and deemph_in_tile else 0
        pad = 45056 if fast and 1024 <= C <= 1792 else 0          # behind the first decimator the front end sees a 256 kSa/s batch: by the station count alone
    front_wgs = n_fo // tile * C
    # --- first decimator: launch_predecim (a stage only where launch_stage_front does not take the capture)
    pk, pt, pw = NO_PREDECIM, 0, 0
    if m > 1 and not pre:
        tpm = (8192 if u8 else 2048) // m
        if fast and n_in % tpm != 0 and n_in % 256 == 0:
            pk, pt = K_PREDECIM_MFMA, 256
        elif fast and n_in % tpm == 0:
            pk, pt = K_PREDECIM_MFMA, tpm
        elif fast:
            pk, pt = K_PREDECIM_PHASES, 512
        else:
            pk, pt = K_PREDECIM, 512
        pw = n_in // pt * C
    # --- de-emphasis stage: launch_stage_deemph
    deemph_wgs = C * ((n_fo // 16 + 63) // 64) if fast else n_fo // 256 * C
    # --- extract: launch_stage_extract, launch_extract_ta, launch_lmr_phase_peek
    lmr_inline = fast and n_est <= 512 and eff <= 6144
    lmr = LMR_INLINE if lmr_inline else (LMR_FAST if fast and n_est <= 512 else LMR_SERIAL)
    et = 256 if n_au % 256 == 0 else 128
    bp = fast and et == 256
    nt, pair = 0, False
    if bp:
        tiles = n_au // 256
        nt = 1
        for v in range(min((tiles + 3) // 4, 0x7fff), 0, -1):
            if (tiles + 4 * v - 1) // (4 * v) * C >= 1536:
                nt = v
                break
        grid = (tiles + 4 * nt - 1) // (4 * nt) * C
        pair = bool(uniform_cutoffs and 4 * nt >= tiles and 2 * tiles <= 4 * 0x7fff and C >= 2 and (pairing == 1 or (pairing == 0 and (C + 1) // 2 >= 1536)))
        if pair:
            nt, grid = (2 * tiles + 3) // 4, (C + 1) // 2
    else:
        grid = n_au // et * C
    # --- RDS: launch_stage_rds
    rds = (K_RDS_SYNC3 if n_au % 256 == 0 else K_RDS_SYNC_FAST) if fast else K_RDS_SYNC
    partials = 2 * (n_au // 256) if fast else 0
    return (int(not fast or keep_taps or n_au % 256 != 0), kernel, source, tile, warm, front_wgs, pad, pk, pt, pw, int(fast), deemph_wgs, int(eff <= 2816), lmr, et, int(bp),
            nt, int(pair), grid, rds, partials)


def stations_to_try(step: int = 0) -> list:
    """Station counts within 3 of every switch (those that go by the block length: at 5120, 8192 and 32768 fm_out samples a block), as the station
    count itself and as the count whose effective batch (x 1.5) is there; with step, every step-th count up to 17000 too."""
    marks = (1, 256, 768, 1024, 1639, 1792, 2816, 3072, 3328, 3584, 4096, 6144, 7168, 12288, 16384, 17000 - 3)
    cs = {c for t in marks for base in (t, t * 2 // 3) for c in range(base - 3, base + 4) if c >= 1}
    if step:
        cs.update(range(1, 17001, step))
    return sorted(cs)
