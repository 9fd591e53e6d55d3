"""The bars of tests/test_gpu_fast_seams.py (also what tests/test_seam_stats_cpu.py proves the detector against).

Each bar is 2 x the worst value measured on an MI355X over the configurations of that test (detuned runs for the ratios and zones, both
pilots for the peaks), as profiles/seams/parity_metrics.json records them; the measured value and the configuration that set it stand
beside each bar.  BARS_OVERRIDE: figures that a group of configurations measures far from the rest are barred there on their own, so
that the rest keep tight ones —
  "deemph"    de-emphasis takes the 38 kHz subcarrier down 20 dB and the L-R error with it, from 1.6e-5 to 9e-7 RMS.  What the block-edge path
              (the block's first 31 outputs, through the fp16 matrix S_old: DESIGN.md section 3) adds where the old and the new L-R offset
              differ, 2e-6 RMS, then stands above the floor.  It is intended structure: that zone is held to its own ABSOLUTE mean square
              there (and is left out of the folds at the shorter periods in every configuration: seam_stats.geometry), and so are the peaks.
  "long_run"  65536-sample blocks at 256 kSa/s make a 6 s run, and in lock the reference's loop drifts inside its float dead zone
              (test_gpu_fast.test_fast_mode_is_within_the_north_star_tolerance_of_the_oracle): a smooth 2e-4 turns of NCO phase, its own peak bar.
"block_first31", "block_first31_moving" (L-R, audio): over the kept pairs both of whose mixed offsets agree with the oracle's (seam_stats.kept_pairs).
"peak_clean" (L-R, audio): the peak over the (station, block) pairs with no offset difference in the block itself or the two in front
(seam_stats.kept_pairs); "peak" over all kept pairs includes the blocks behind a flipped phase estimate of the reference's tracker.
"""
import copy

from seam_stats import STREAMS

# BEGIN MEASURED
BARS = {
    "fm_out_iq": {
        "peak": 2.1e-05,        # measured 1.07e-05 (1024k_b65536_split_detuned)
        "ratio": {
            "16": 2.0,        # measured 1.01 (256k_b9216_detuned)
            "predecim": 2.2,        # measured 1.1 (1024k_b65536_split_detuned)
            "tile": 2.4,        # measured 1.19 (1024k_b65536_u8_detuned)
            "1024": 2.2,        # measured 1.11 (256k_b16384_u8_detuned)
        },
        "zone": {
            "block_first192": 2.1,        # measured 1.03 (1024k_b65536_split_detuned)
            "block_last64": 2.1,        # measured 1.03 (1024k_b65536_split_detuned)
            "tile_first64": 2.0,        # measured 1.02 (1024k_b65536_u8_detuned)
            "tile_last64": 2.0,        # measured 1.01 (256k_b65536_detuned)
            "tile_first128": 2.0,        # measured 1.01 (256k_b10240_deemph_detuned)
        },
    },
    "pll_dt": {
        "peak": 0.00015,        # measured 7.36e-05 (256k_b16384_u8_detuned)
        "ratio": {
            "16": 2.0,        # measured 1 (256k_b16384_u8_detuned)
            "16_detrended": 5.9,        # measured 2.97 (1024k_b65536_split_detuned)
            "span": 2.0,        # measured 1 (256k_b16384_u8_detuned)
            "span_detrended": 10.0,        # measured 5.09 (1024k_b65536_u8_detuned)
        },
        "zone": {
            "block_first_span": 2.0,        # measured 0.991 (256k_b2048_detuned)
            "span_first16": 2.0,        # measured 1 (1024k_b12288_u8_detuned)
            "span_last16": 2.0,        # measured 1 (256k_b16384_u8_detuned)
        },
    },
    "lpr": {
        "peak": 9.7e-06,        # measured 4.86e-06 (1024k_b65536_split_pilot19000)
        "ratio": {
            "16": 2.4,        # measured 1.21 (1024k_b65536_split_detuned)
            "tile": 2.6,        # measured 1.28 (2048k_b131072_detuned)
            "4tiles": 2.8,        # measured 1.41 (256k_b10240_deemph_detuned)
        },
        "zone": {
            "block_first31": 2.0,        # measured 1.02 (1024k_b65536_split_detuned)
            "block_last_tile": 2.0,        # measured 1.02 (1024k_b65536_split_detuned)
            "tile_first47": 2.0,        # measured 1.02 (256k_b16384_cf32_detuned)
        },
    },
    "lmr": {
        "peak": 0.0013,        # measured 0.000635 (1024k_b65536_u8_detuned)
        "peak_clean": 0.00031,        # measured 0.000154 (2048k_b131072_detuned)
        "ratio": {
            "16": 2.8,        # measured 1.42 (1024k_b12288_u8_detuned)
            "tile": 4.1,        # measured 2.04 (1024k_b12288_u8_detuned)
            "4tiles": 4.5,        # measured 2.23 (256k_b9216_detuned)
        },
        "zone": {
            "block_first31": 2.5,        # measured 1.24 (1024k_b12288_u8_detuned)
            "block_first31_moving": 4.8,        # measured 2.4 (1024k_b12288_u8_detuned)
            "block_last_tile": 3.3,        # measured 1.66 (1024k_b12288_u8_detuned)
            "tile_first47": 2.1,        # measured 1.06 (1024k_b12288_u8_detuned)
        },
    },
    "audio": {
        "peak": 0.0036,        # measured 0.0018 (1024k_b65536_u8_detuned)
        "peak_clean": 0.00087,        # measured 0.000436 (2048k_b131072_detuned)
        "ratio": {
            "16": 2.8,        # measured 1.41 (1024k_b12288_u8_detuned)
            "tile": 4.0,        # measured 2.02 (1024k_b12288_u8_detuned)
            "4tiles": 4.4,        # measured 2.22 (256k_b9216_detuned)
        },
        "zone": {
            "block_first31": 2.5,        # measured 1.24 (1024k_b12288_u8_detuned)
            "block_first31_moving": 4.7,        # measured 2.37 (1024k_b12288_u8_detuned)
            "block_last_tile": 3.3,        # measured 1.65 (1024k_b12288_u8_detuned)
            "tile_first47": 2.1,        # measured 1.06 (1024k_b12288_u8_detuned)
        },
    },
}
BARS_OVERRIDE = {
    "deemph": {
        "lmr": {
            "peak": 4.6e-05,        # measured 2.32e-05 (256k_b10240_deemph_detuned)
            "peak_clean": 3.9e-05,        # measured 1.93e-05 (256k_b10240_deemph_detuned)
            "zone_ms": {
                "block_first31": 7.2e-12,        # measured 3.6e-12 (256k_b10240_deemph_detuned)
                "block_first31_moving": 1.1e-11,        # measured 5.49e-12 (256k_b10240_deemph_detuned)
            },
        },
        "audio": {
            "peak": 0.00013,        # measured 6.57e-05 (256k_b10240_deemph_detuned)
            "peak_clean": 0.00011,        # measured 5.45e-05 (256k_b10240_deemph_detuned)
            "zone_ms": {
                "block_first31": 6.5e-11,        # measured 3.27e-11 (256k_b10240_deemph_detuned)
                "block_first31_moving": 9.6e-11,        # measured 4.79e-11 (256k_b10240_deemph_detuned)
            },
        },
    },
    "long_run": {
        "pll_dt": {
            "peak": 0.00042,        # measured 0.000212 (256k_b65536_detuned)
        },
    },
}
# END MEASURED


def bars_for(overrides=()):
    """The bars per stream of a configuration that names `overrides` (keys of BARS_OVERRIDE)."""
    out = copy.deepcopy(BARS)
    for k in STREAMS:
        out.setdefault(k, {"peak": 0.0, "ratio": {}, "zone": {}})
    for name in overrides:
        for stream, sub in BARS_OVERRIDE.get(name, {}).items():
            for key, val in sub.items():
                if isinstance(val, dict):
                    out[stream].setdefault(key, {}).update(val)
                else:
                    out[stream][key] = val
    return out
