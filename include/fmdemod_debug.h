/* fmdemod_debug.h — test, self-check and profiling hooks of libfmdemod.so.
 *
 * NOT part of the drop-in boundary (include/fmdemod.h): nothing here has a counterpart in the reference's demodulator API.
 * tests/ use the self-tests to compare the device math with the host libm the reference links; bench.py uses the profiling
 * hooks for its roofline figures.  Results of the demodulator never depend on any of these calls.
 */
#ifndef FMDEMOD_DEBUG_H
#define FMDEMOD_DEBUG_H

#include "fmdemod.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-kernel timing with HIP events recorded on the processing stream (for bench.py's roofline figures).
 * on = 1: every fmd_process_* call brackets each kernel of the sequence with events; on = 2: k_pilot_pll (the dominant
 * kernel) of every block, the other kernels of every 4th block — the brackets are extra queue packets between dependent
 * kernels and cost the pipelined step a few percent; fmd_profile_read synchronises, accumulates and clears them. */
typedef struct {
    char   name[32];     /* kernel name as it appears in rocprofv3 kernel traces (prefix match) */
    double total_ms;     /* sum of launch durations since the last read */
    int    launches;
} fmd_kernel_time;
/* Self-test hook: evaluates the kernels' atan2f on the device for n host-side (y, x) pairs, so tests can compare
 * the device math bit-for-bit with the host libm the reference links (std::atan2, reference fm_demod.cpp:40). */
int fmd_selftest_atan2(const float* y, const float* x, float* out, size_t n);
/* Same for the table-driven form the discriminator (k_front) uses: identical values, fewer issued instructions. */
int fmd_selftest_atan2_table(const float* y, const float* x, float* out, size_t n);
/* ... and its variant for u8 IQ at 256 kSa/s, whose operands are the integers -127..128 (only 0/0 is special there). */
int fmd_selftest_atan2_table_u8(const float* y, const float* x, float* out, size_t n);
/* Same for the short form k_pilot_pll's phase detector uses on a locked loop: out[i] is only meaningful where ok[i] != 0, and
 * there it must equal atan2f(y[i], x[i]) bit-for-bit (DESIGN.md "Pilot PLL"). */
int fmd_selftest_atan2_small(const float* y, const float* x, float* out, uint8_t* ok, size_t n);

/* The FMD_FLAG_FAST_MATH primitives evaluated on the device, for accuracy checks against float64 on the host:
 * kind 0: out = fast atan2(a, b); kind 1: out = sin(2 pi a) (hardware, argument in turns); kind 2: out = cos(2 pi a);
 * kind 3: out = atan2(a, b) / 2 pi, the six-coefficient form of the discriminator and the pilot loop's phase detector. */
int fmd_selftest_fast_math(int kind, const float* a, const float* b, float* out, size_t n);

/* Host-only (no GPU needed): the tables of the tolerance mode's span-wise pilot PLL (fm-radio_amd/csrc/fmd_tables.h PllSpanTab) as
 * the library designs them for fs_baseband — w [5][128] weights of the held-frequency error sequence (rows: loop filter, integrator,
 * phase deviation at samples 41, 84, 127), s [5][8] weights of the state (lpf, I, e1, e2, r0), minv [3][4] cubic fit, misc[0] = the
 * quadrature factor, misc[1] = kappa.  tests/test_span_design.py checks them against an independent float64 restatement. */
int fmd_design_pll_span(int fs_baseband, float* w, float* s, float* minv, float* misc2);
/* ... and of the round-4 form that evaluates the loop's phase detector at 8 points of a span (PllSparseTab, k_pll_sparse): taps [2][32]
 * (real, imaginary weight of a point's 32 input samples), cplx [19][2] = rot[8], scan[3], carry[8] as (re, im), rows [2][8] = wsum, wmom
 * (5 used each), sw [5][132] suffix sums of the weight rows, misc8 = phi0, inv_s2, nbar, kappa, pw_scale, kap2 (re, im), 0.
 * tests/test_span_design.py checks them against a float64 model of the reference's peak filter and loop. */
int fmd_design_pll_sparse(int fs_baseband, float* taps, float* cplx, float* rows, float* sw, float* misc8);

/* Taps of k_extract_bp's composite band-pass FIRs (fmd_kernels_bp.inc: the harmonic mixer's carrier and the Hilbert FIR folded into the
 * decimating FIR): g2 [2][192] = (real, imaginary) taps of the L-R FIR for an L-R cut-off of cutoff_hz, g3 [2][192] of the RDS FIR.
 * tests/test_bandpass_design.py checks them against the reference's order of operations in float64. */
int fmd_design_extract_bp(int fs_baseband, int cutoff_hz, float* g2, float* g3);

/* The tolerance mode's table for the discriminator's wrap at exactly half a turn on u8 captures (fmd_kernels.hip wrap_tie_u8): 65536 bits,
 * bit (y_raw << 8 | x_raw) = 1 when the reference's wrapped phase difference from sample (x_raw, y_raw) to one in exactly the opposite direction
 * is +pi.  tests/test_wrap_tie.py checks it against glibc's atan2f. */
int fmd_design_wrap_tie(uint32_t* bits2048);

/* Counters of k_pilot_pll's frequency speculation since creation / the last reset (DESIGN.md "Pilot PLL"):
 * out8[0] = 128-sample chunks, summed over wavefronts (4 channels each); out8[1] = of those, chunks run with the plain serial
 * iteration (wavefront out of lock); out8[2] = spans redone with the reference forms (a short form outside its domain);
 * out8[3] = spans, out8[4] = samples committed, both summed over channels (ratio = samples per 16-sample span);
 * out8[5] = spans run in the sequence form (a loop out of lock: the span speculates on the sequence of frequency words), summed over wavefronts;
 * out8[6], out8[7] = shader-clock cycles and 100 MHz real-time ticks of one wavefront per launch (ratio x 100 = core MHz).
 * Results never depend on any of them; they explain k_pilot_pll's duration. */
int fmd_get_spec_stats(fmd_handle h, uint64_t* out8, int reset);

/* on = 0: off; 1: timing events on every kernel of every block; 2: the dominant kernel every block, the others every 4th;
 * 3: every kernel of every 4th block plus the dominant kernel of the block behind it (what bench.py uses: ~1 % of the step) */
int fmd_profile_enable(fmd_handle h, int on);
/* 1.024 / 2.048 MSa/s, tolerance mode: on = 1 runs the first decimator and the front end as the two kernels they were (k_predecim_mfma,
 * k_front_mfma with fm_in through HBM) instead of k_front_pre_mfma; results are bit-identical either way (tests/test_gpu_fast.py).
 * Between blocks only. */
int fmd_debug_split_front(fmd_handle h, int on);
int fmd_profile_read(fmd_handle h, fmd_kernel_time* out, int cap, int* n_out);
/* Exact mode, test hook: the batch sizes up to which the pilot PLL runs as the time-parallel kernel with 16 lanes a station (default 3584) and as the
 * time-parallel kernel at all (default 7168; the low-work kernel above).  Beyond either the choice follows what is out of lock:
 * 8 lanes / the low-work kernel while every loop holds lock, 16 lanes (up to 4096 stations) / the time-parallel kernel while some do not.  With small
 * values a small batch exercises the switches (tests/test_gpu_parity.py); results are bit-identical whatever kernel runs. */
int fmd_debug_pll_adaptive(fmd_handle h, int k16_max_channels, int time_parallel_max_channels);
/* Host-only (no GPU needed): which kernels the library picks for a configuration (fm-radio_amd/csrc/fmd_plan.h, the one place where batch sizes
 * decide).  k16_max_channels, time_parallel_max_channels: both negative = the defaults, both >= 0 = as after fmd_debug_pll_adaptive with them
 * (FMD_ERR_ARG where that hook refuses).  unlocked_now: whether loops ran out of lock in the last blocks, which pll_kernel depends on.
 * pll_kernel is the exact mode's; the tolerance mode runs k_pll_sparse whatever it says.  tests/test_plan_cpu.py compares every field with a
 * restatement of the rules and aims the batch sizes of tests/test_gpu_every_station.py at the switches. */
enum { FMD_PLL_KERNEL_LOW_WORK = 0, FMD_PLL_KERNEL_TIME_PARALLEL_16 = 1, FMD_PLL_KERNEL_TIME_PARALLEL_8 = 2 };
typedef struct {
    int effective_channels;   /* stations, x 1.5 at 1.024 and 2.048 MSa/s: what most switches compare */
    int pilot_power_rows;     /* k_pilot_power<true> */
    int pll_k_adaptive;       /* the pilot-PLL kernel follows what is out of lock */
    int pll_chained;          /* consecutive k_pilot_pll launches hand over per wavefront */
    int pll_waves;            /* wavefronts the hand-over array is allocated for */
    int lmr_inline;           /* k_extract integrates the L-R phase itself */
    int lazy_capable;         /* fmd_submit_*: the extract stage waits for the next block's front end */
    int front_lds_pad;        /* bytes of extra dynamic LDS of k_front_mfma */
    int front_big_tile;       /* cf32: 2048-output front-end tiles where the block length allows */
    int extract_auto_pair;    /* k_extract_bp<2> where its other conditions hold */
    int pll_kernel;           /* FMD_PLL_KERNEL_* */
} fmd_plan_info;
int fmd_debug_plan(const fmd_config* cfg, int k16_max_channels, int time_parallel_max_channels, int unlocked_now, fmd_plan_info* out);
/* Host-only (no GPU needed): each stage's kernel form and launch geometry for a configuration (fm-radio_amd/csrc/fmd_plan.h BlockPlan: what the
 * block length, the input type — u8 != 0: fmd_process_u8, else cf32 — and the run-time facts decide on top of fmd_debug_plan's fields; the stage
 * launchers read it and decide nothing).  facts: what the controls and the debug hooks leave behind — a station's de-emphasis as a stage of its own, or
 * (tolerance mode) inside the front end's tile; fmd_debug_split_front; every station with the same audio cut-offs; fmd_debug_extract_pairing's mode.
 * tests/test_plan_cpu.py compares every field with a restatement of the rules (tests/plan_model.py). */
typedef struct { int any_deemph, deemph_in_tile, split_front, uniform_cutoffs, extract_pairing; } fmd_plan_facts;
enum { FMD_FRONT_K_FRONT = 0, FMD_FRONT_K_FRONT_MFMA = 1, FMD_FRONT_K_FRONT_PRE_MFMA = 2 };
enum { FMD_FRONT_INPUT_CF32 = 0, FMD_FRONT_INPUT_U8 = 1, FMD_FRONT_INPUT_FM_IN = 2, FMD_FRONT_INPUT_PHASES = 3 };
enum { FMD_PREDECIM_NONE = 0, FMD_PREDECIM_K_PREDECIM = 1, FMD_PREDECIM_K_PREDECIM_PHASES = 2, FMD_PREDECIM_K_PREDECIM_MFMA = 3 };
enum { FMD_LMR_PHASE_INLINE = 0, FMD_LMR_PHASE_FAST = 1, FMD_LMR_PHASE_SERIAL = 2 };
enum { FMD_RDS_K_RDS_SYNC = 0, FMD_RDS_K_RDS_SYNC_FAST = 1, FMD_RDS_K_RDS_SYNC3 = 2 };
typedef struct {
    int iq_streams;           /* the handle materialises fm_out_iq / pll_dt */
    int front_kernel;         /* FMD_FRONT_K_* */
    int front_input;          /* FMD_FRONT_INPUT_*: the capture, or behind a first-decimator stage fm_in as samples or as phases */
    int front_tile;           /* fm_out samples per workgroup: 512, 1024, 2048 */
    int front_warmup;         /* k_front_mfma: samples the in-tile de-emphasis starts early (0, 128) */
    int front_workgroups;     /* stations x tiles (without the pilot stage's workgroups that may ride in the launch) */
    int front_lds_pad;        /* bytes of extra dynamic LDS */
    int predecim_kernel;      /* FMD_PREDECIM_*: NONE exactly when the front end takes the capture */
    int predecim_tile;        /* fm_in samples per workgroup */
    int predecim_workgroups;
    int deemph_pilot_sums;    /* the de-emphasis stage is k_deemphasis + k_pilot_sums, not k_deemphasis + k_hilbert */
    int deemph_workgroups;    /* of the second kernel of the pair */
    int pilot_power_rows;     /* k_pilot_power<true> */
    int lmr_phase;            /* FMD_LMR_PHASE_* */
    int extract_tile;         /* audio samples per tile: 128, 256 */
    int extract_bp;           /* k_extract_bp, not k_extract */
    int extract_nt;           /* k_extract_bp: tiles per wavefront */
    int extract_pair;         /* k_extract_bp<2> */
    int extract_grid_x;
    int rds_kernel;           /* FMD_RDS_K_* */
    int rds_partials;         /* partial sums of the block's RDS power per station */
} fmd_block_plan_info;
int fmd_debug_block_plan(const fmd_config* cfg, const fmd_plan_facts* facts, int u8, fmd_block_plan_info* out);
/* Tolerance mode: k_extract_bp with two stations per workgroup (the tap tables and the block edge's matrix fetched once for both; results bit-identical):
 * 0 = where it pays (3072 stations and more with equal cut-offs, the default), 1 = wherever possible (so that tests reach it with a few stations), 2 = never. */
int fmd_debug_extract_pairing(fmd_handle h, int mode);

#ifdef __cplusplus
}
#endif
#endif
