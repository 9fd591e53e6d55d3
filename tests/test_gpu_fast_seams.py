"""GPU tests (pytest -m gpu) that bound the tolerance mode (FMD_FLAG_FAST_MATH) in PEAK and BY POSITION, not only in RMS.

test_gpu_fast.py, test_gpu_scale.py, test_gpu_long.py, test_gpu_realistic.py and test_gpu_every_station.py hold the mode to RMS distances over
at least a whole block.  Its kernels are tiled, and nearly all their special code sits at tile, span and block edges: a wrong halo index, a
tap off a table's zero padding, an fp16 row of the block-edge matrix, a span hand-over one sample late.  Each leaves ONE bad sample (or one
short zone) per period, which an RMS bar B over a period of T samples passes up to A = B sqrt(T).  Here the error against the CPU oracle
(handed the library's coefficients, as test_gpu_fast._compare does) is folded by position inside every period the kernels have
(tests/seam_stats.py: geometry() cites where each comes from) and bound by
  peak                  max |e| per stream,
  worst-position ratio  the worst position's mean square over the median position's, per period,
  zone ratio            the same for the named edge zones (and for whole-block periods, where single positions pool too few samples).
Every configuration runs with the pilot at exactly 19 000 Hz and detuned to 19 003.7 Hz.  At 19 000 Hz the pilot makes exactly 19 cycles per
128-sample span, so pilot-locked arithmetic error is itself periodic in 16 / 128 / 1024 samples and looks like a seam: that run is recorded
and bound on peak only; the detuned run decides the ratios.

The bars (tests/seam_bars.py) are 2 x the worst value measured on an MI355X over the configurations below (profiles/seams/parity_metrics.json
holds every figure per configuration; the measured worst is quoted beside each bar).  Two things hold whatever was measured, and are asserted on the
GPU's own output in every detuned run:
  * a defect of A / 4 (A = B sqrt(T), B today's RMS bar of the stream) injected on the host at position 0, T / 2 and T - 1 of every period
    shorter than the block fails the check;
  * a zone defect of B sqrt(block / |Z|) / 4 over the block's first 31 audio outputs (lpr, lmr, audio) and over the block's first span
    (pll_dt) fails it.
RDS symbols are not folded: their spacing is irregular, and test_gpu_fast.soft_symbol_stats looks at single symbols.
"""
import numpy as np
import pytest

import oraclelib as O
import seam_stats as S
import synth
from gpu_parity import lib_coeffs_to_oracle, oracle_controls, run_gpu
from seam_bars import bars_for
from seam_stats import DETUNED_HZ
from test_gpu_fast import record_parity_metrics

pytestmark = pytest.mark.gpu

MIN_MOVING_EDGES = 16      # kept block edges that mix two offsets more than 0.01 apart: 31 outputs each, their zone mean then has 6 % of spread

# configuration -> fs, block, u8, de-emphasis (50 us on every station), first decimator as a kernel of its own, stations
FORMS = {
    # 1024-output front tiles (u8: 2048), 256-sample extract tiles, L-R phase integrated inside the extract stage
    "256k_b16384_cf32": dict(fs=256_000, bs=16384, n_ch=8),
    "256k_b16384_u8": dict(fs=256_000, bs=16384, u8=True, n_ch=8),
    # 512-sample front tiles, 128-sample extract tiles
    "256k_b9216": dict(fs=256_000, bs=9216, n_ch=8),
    # tiles that do not fill a workgroup: 1, 3 and 6 extract tiles a block
    "256k_b2048": dict(fs=256_000, bs=2048, n_ch=8),
    "256k_b6144": dict(fs=256_000, bs=6144, n_ch=8),
    "256k_b12288": dict(fs=256_000, bs=12288, n_ch=8),
    # the L-R phase integrated by a kernel of its own behind the extract stage: 820 estimates a block are more than kLmrInlineMax = 512, so
    # launch_stage_extract (fmd_kernels.hip) launches the serial k_lmr_phase.  (k_lmr_phase_fast runs behind the extract stage only for blocks of up to
    # 512 estimates in batches of more than kLmrInlineMaxEff = 6144 effective stations, fmd_plan.cpp: NOT covered here.  Every configuration with
    # up to 512 estimates runs that kernel once a block through the lmr_phase getter, launch_lmr_phase_peek, whose value decides the pairs kept.)
    "256k_b65536": dict(fs=256_000, bs=65536, n_ch=8, override=("long_run",)),
    # de-emphasis inside the front tile (1024- and, at 10240, again 1024-sample tiles over 5 tiles; 256-sample extract tiles)
    "256k_b16384_deemph": dict(fs=256_000, bs=16384, deemph=True, n_ch=8, override=("deemph",)),
    "256k_b10240_deemph": dict(fs=256_000, bs=10240, deemph=True, n_ch=8, override=("deemph",)),
    # the fused first decimator k_front_pre_mfma
    "1024k_b65536_cf32": dict(fs=1_024_000, bs=65536, n_ch=6),
    "1024k_b65536_u8": dict(fs=1_024_000, bs=65536, u8=True, n_ch=6),
    "2048k_b131072": dict(fs=2_048_000, bs=131072, n_ch=6),
    # k_predecim_mfma on its own: 2048-input tiles (fmd_debug_split_front) and 256-output tiles (u8 blocks that are no multiple of its tile)
    "1024k_b65536_split": dict(fs=1_024_000, bs=65536, split_front=True, n_ch=6),
    "1024k_b12288_u8": dict(fs=1_024_000, bs=12288, u8=True, n_ch=6),
}


def n_blocks(fs, bs):
    """26 blocks, or as many as 1.5 s take (26: with the block's first 31 outputs left out of the shorter folds, the four-tile fold of a 16384-sample
    block, two folds a block, pools 8 stations x 26 = 208 >= MIN_POOL samples at those positions).  The oracle's pilot loop needs 0.4-0.5 s to acquire the detuned pilot, whatever the block length, and
    while it does the L-R samples turn through zero and the sign decisions of the phase estimates (test_gpu_fast.lmr_audio_excess) fall
    differently far more often than in lock: two thirds of the run behind the acquisition keep the dropped (station, block) pairs under the cap."""
    return max(26, -(-3 * fs // (2 * bs)))


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    import torch
    assert torch.cuda.is_available()
    return p


def oracle_side(form, pilot_hz):
    """The captures of one configuration (one station per channel number, the same seed for both pilots) and their block count."""
    f = FORMS[form]
    fs, bs, u8 = f["fs"], f["bs"], f.get("u8", False)
    nb = n_blocks(fs, bs)
    conv = synth.to_u8 if u8 else synth.to_cf32
    caps = np.stack([conv(synth.fm_capture(nb * bs, fs=float(fs), seed=9900, channel=c, pilot_hz=pilot_hz)["iq"]) for c in range(f["n_ch"])])
    return caps, nb


def run_form(pkg, form, pilot_hz):
    """Tolerance mode on the GPU against the oracle: error arrays per stream, the (station, block) pairs kept for L-R / audio, and run facts."""
    f = FORMS[form]
    fs, bs, u8 = f["fs"], f["bs"], f.get("u8", False)
    caps, nb = oracle_side(form, pilot_hz)
    ctl = None
    if f.get("deemph"):
        from fm_radio_amd.capi import default_controls
        ctl = default_controls()
        ctl.use_deemphasis = 1
        ctl.deemphasis_tus = 50
    g = run_gpu(pkg, caps, bs, fs, fast_math=True, controls=ctl, split_front=f.get("split_front", False))
    want = {k: [] for k in S.STREAMS + ("lmr_phase",)}
    lock = []
    for c in range(caps.shape[0]):
        o = O.run_chain(caps[c], bs, fs, u8=u8, controls=oracle_controls(ctl) if ctl is not None else None, coeffs=lib_coeffs_to_oracle(g["coeffs"][c]),
                        streams=list(S.STREAMS) + ["lmr_phase", "pll_raw_err"])
        for k in want:
            want[k].append(o[k].reshape(-1))
        tail = o["pll_raw_err"].astype(np.float64).reshape(nb, -1)[-max(2, nb // 8):]
        lock.append(float(np.sqrt((tail ** 2).mean())))
    errs = {k: S.stream_error(k, g[k], np.stack(want[k]), nb) for k in S.STREAMS}
    keep, moving, clean, edge = S.kept_pairs(np.asarray(g["lmr_phase"]).reshape(caps.shape[0], -1)[:, :nb], np.stack(want["lmr_phase"])[:, :nb])
    first31 = S.squared(errs["lmr"])[:, :, :31].mean(axis=2)          # the block-edge path's outputs: by whether the two offsets it mixes differ
    facts = {"blocks": nb, "stations": int(caps.shape[0]), "oracle_lock_rms_rad": max(lock), "dropped_share": float(1.0 - keep.mean()),
             "dropped_stations_by_block": " ".join(str(int(v)) for v in (~keep).sum(axis=0)), "moving_share_of_all": float(moving.mean()),
             "moving_share_of_kept": float(moving[keep].mean()), "moving_kept_edges": int((moving & keep).sum()), "moving_edge_pairs": int((moving & edge).sum()), "edge_share": float(edge.mean()),
             "clean_share": float(clean.mean()),
             "lmr_first31_ms_kept_moving": float(first31[keep & moving].mean()) if (keep & moving).any() else None,
             "lmr_first31_ms_kept_still": float(first31[keep & ~moving].mean()) if (keep & ~moving).any() else None}
    return errs, (keep, moving, clean, edge), facts


@pytest.mark.parametrize("pilot_hz", [19000.0, DETUNED_HZ], ids=["pilot19000", "detuned"])
@pytest.mark.parametrize("form", list(FORMS))
def test_fast_mode_error_is_bound_in_peak_and_by_position(pkg, form, pilot_hz):
    """One configuration of FORMS against the oracle: peak per stream (both pilots), worst-position and zone ratios at every period of its
    kernels (detuned pilot), and on the detuned run the injected defects that today's RMS bars pass must fail (module docstring).  The oracle
    alone must hold lock on the capture; at most a quarter of the (station, block) pairs may be dropped for L-R and audio."""
    f = FORMS[form]
    geo = S.geometry(f["fs"], f["bs"], f.get("u8", False), f.get("deemph", False), f.get("split_front", False))
    errs, (keep, moving, clean, edge), facts = run_form(pkg, form, pilot_hz)
    detuned = pilot_hz != 19000.0
    bars = bars_for(f.get("override", ()))
    figs = {k: S.figures(errs[k], geo[k], keep, moving=moving, clean=clean, edge=edge) if k in ("lmr", "audio") else S.figures(errs[k], geo[k]) for k in S.STREAMS}
    doc = dict(facts, geometry={k: geo[k] for k in ("n_fm_out", "n_audio", "front_tile", "extract_tile")}, streams=figs)
    print(form, pilot_hz, facts)
    for k in S.STREAMS:
        print("  %-9s rms %.3g peak %.3g clean %.3g ratio %s zone %s" % (k, figs[k]["rms"], figs[k]["peak"], figs[k].get("peak_clean", 0.0), {a: None if b is None else round(b, 3) for a, b in figs[k]["ratio"].items()},
                                                         {a: round(b, 3) for a, b in figs[k]["zone"].items()}))
    # the reference side: the oracle alone holds lock on the capture, and the blocks kept for L-R / audio still exercise the block-edge path
    assert facts["oracle_lock_rms_rad"] < 0.25, facts
    assert facts["dropped_share"] <= 0.25, facts
    # at least half of the kept block edges mix two offsets more than 0.01 apart — wherever the capture allows it: where the ORACLE's own offset
    # moves that much on fewer than half of ALL edges (decided on the CPU side alone: 8 ms blocks of 25 estimates, 256 ms blocks behind which
    # the tracker has settled, most 19 000 Hz runs) no choice of kept pairs could.  So that the first-31 zone is judged on the path it polices in
    # every configuration, L-R and audio also carry that zone over the MOVING edges only ("block_first31_moving"), and there must be at least
    # MIN_MOVING_EDGES of them.  (Both first-31 zones of L-R and audio count the kept pairs whose offset of TWO blocks back agrees with the oracle's as
    # well, seam_stats.kept_pairs' `edge`: those outputs mix that offset too, and a flipped estimate there is the same documented discontinuity.)
    if facts["moving_share_of_all"] >= 0.5:
        assert facts["moving_share_of_kept"] >= 0.5, facts
    assert facts["moving_edge_pairs"] >= MIN_MOVING_EDGES, facts
    bad = []
    for k in S.STREAMS:
        v = S.violations(k, figs[k], bars[k])
        bad += v if detuned else [x for x in v if x[1].startswith("peak")]
    if detuned:
        misses, smallest, zones = S.sensitivity(errs, geo, keep, bars, moving, edge)
        doc["smallest_caught_multiple_of_A"] = smallest
        doc["zone_defects_caught"] = zones
        print("  smallest caught multiple of A:", smallest, zones)
    record_parity_metrics(f"seams_{form}_{'detuned' if detuned else 'pilot19000'}", doc)
    assert not bad, bad
    if detuned:
        assert not misses, misses
