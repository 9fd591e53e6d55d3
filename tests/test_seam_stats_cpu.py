"""The peak / by-position detector of tests/seam_stats.py, proven on the CPU before it judges a kernel (tests/test_gpu_fast_seams.py).

The "tolerance-mode output" here is a surrogate: the oracle's own output plus white noise at the RMS the tolerance mode measures per stream
(profiles/round6/parity_metrics.json), once plain and once scaled by the local signal level.  Shown:
  1. without a defect every ratio stays near 1 (the spread is stated in the test);
  2. every defect of the list the GPU test injects is flagged, at the amplitude required there, by the ratio and zone bars the GPU test uses;
  3. the same defected arrays still pass today's RMS bars (rms, lmr_audio_excess <= 1) — the gap this closes.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import oraclelib as O
import seam_stats as S
import synth
from conftest import rms
from test_gpu_fast import lmr_audio_excess
from seam_bars import BARS
from seam_stats import DETUNED_HZ, sensitivity

ROOT = Path(__file__).resolve().parent.parent
FS, BS, NB, N_ST = 256_000, 16384, 26, 8
GEO = S.geometry(FS, BS)


@pytest.fixture(scope="module")
def oracle_run():
    """Eight stations x 26 blocks of the oracle (1.2 s on the CPU), shared and left unchanged."""
    runs = []
    for c in range(N_ST):
        cap = synth.to_cf32(synth.fm_capture(NB * BS, fs=float(FS), seed=9900, channel=c, pilot_hz=DETUNED_HZ)["iq"])
        runs.append(O.run_chain(cap, BS, FS, u8=False, streams=list(S.STREAMS) + ["lmr_phase"]))
    return runs


def measured_rms():
    m = json.loads((ROOT / "profiles" / "round6" / "parity_metrics.json").read_text())["fast_vs_oracle_12_blocks_fs256000_u8"]
    return {k: float(m[k]) for k in S.STREAMS}


def local_level(x, width=64):
    """|x| smoothed over `width` samples, over its own RMS: what an error proportional to the signal is scaled by."""
    p = np.convolve(np.asarray(x, np.float64) ** 2, np.ones(width) / width, mode="same")
    return np.sqrt(p / p.mean())


@pytest.fixture(scope="module", params=["plain", "scaled"])
def surrogate(request, oracle_run):
    """e[S, nb, n] per stream: white noise at the measured RMS (per real sample), plain or scaled by the local level of the oracle's stream."""
    rng = np.random.default_rng(77)
    sig = measured_rms()
    errs = {}
    for k in S.STREAMS:
        want = np.stack([r[k].reshape(-1) for r in oracle_run]).astype(np.float64)
        noise = sig[k] * rng.standard_normal(want.shape)
        if request.param == "scaled" and k != "pll_dt":          # (pll_dt is a sawtooth phase: no level to follow)
            noise *= np.stack([local_level(w) for w in want])
        errs[k] = S.stream_error(k, want + noise, want, NB)
    return request.param, errs


def test_geometry_of_the_configurations():
    g = S.geometry(256_000, 16384)
    assert (g["n_fm_out"], g["n_audio"], g["front_tile"], g["extract_tile"]) == (8192, 2048, 1024, 256)
    assert S.geometry(256_000, 16384, u8=True)["front_tile"] == 2048 and S.geometry(256_000, 16384, u8=True, deemph=True)["front_tile"] == 1024
    g = S.geometry(256_000, 9216)
    assert (g["front_tile"], g["extract_tile"], g["lmr"]["periods"]["4tiles"]) == (512, 128, 512)
    assert "4tiles" not in S.geometry(256_000, 2048)["lmr"]["periods"]
    assert S.geometry(1_024_000, 65536)["front_tile"] == 1024 and "predecim" not in S.geometry(1_024_000, 65536)["fm_out_iq"]["periods"]
    assert S.geometry(1_024_000, 65536, split_front=True)["fm_out_iq"]["periods"]["predecim"] == 256
    assert S.geometry(1_024_000, 65536, u8=True, split_front=True)["fm_out_iq"]["periods"]["predecim"] == 1024
    g = S.geometry(1_024_000, 12288, u8=True)
    assert (g["front_tile"], g["extract_tile"], g["fm_out_iq"]["periods"]["predecim"]) == (512, 128, 128)


def test_fold_inject_and_ratios_on_known_arrays():
    e = np.zeros((2, 3, 40))
    d = S.inject(e, 16, 0.5, 3)
    assert np.array_equal(np.nonzero(d[1, 2])[0], [3, 19, 35]) and not e.any()
    prof, cnt = S.fold_profile(S.squared(d), 16)
    assert np.array_equal(cnt, [18] * 8 + [12] * 8) and prof[3] == 0.25 and prof.sum() == 0.25
    keep = np.array([[True, False, True], [False, False, True]])
    assert S.fold_profile(S.squared(d), 16, keep)[1][0] == 9
    st = S.inject(np.zeros((1, 1, 64, 2)), 64, 2.0, 0, 16)
    assert S.squared(st)[0, 0, :16].tolist() == [4.0] * 16 and st[..., 1].sum() == 0
    cx = S.stream_error("fm_out_iq", np.array([[1.0, 2.0, 3.0, 5.0]]), np.array([[1.0, 1.0, 1.0, 1.0]]), 1)
    assert cx.shape == (1, 1, 2) and S.squared(cx)[0, 0].tolist() == [1.0, 20.0] and S.peak(S.squared(cx)) == np.sqrt(20.0)
    assert abs(S.stream_error("pll_dt", np.array([[0.99]]), np.array([[0.01]]), 1)[0, 0, 0] + 0.02) < 1e-12
    assert S.worst_position_ratio(np.ones(4), np.array([199] * 4)) == (None, None)
    assert S.zone_ratio(np.array([3.0] * 16 + [1.0] * 48), 0, 16) == 3.0
    # the block's first samples left out of a fold: they count at no position
    prof, cnt = S.fold_profile(S.squared(S.inject(np.zeros((2, 3, 64)), 64, 1.0, 0, 4)), 16, skip_first=4)
    assert cnt.tolist() == [18] * 4 + [24] * 12 and prof.sum() == 0.0
    # the zone over the moving kept pairs, a zone held to its absolute mean square, the clean peak
    e = S.inject(np.zeros((2, 2, 64)), 64, 0.1, 32, 64)
    e[0, 1, :31] += 0.3
    keep = np.array([[True, True], [True, False]]); moving = np.array([[False, True], [True, True]]); clean = np.array([[True, False], [True, True]])
    fig = S.figures(e, {"periods": {"block": 64}, "zones": [], "edge_zones": [("block_first31", 0, 31, False), ("block_first31_moving", 0, 31, True)]},
                    keep, moving=moving, clean=clean, edge=keep)
    assert fig["moving_edge_pairs"] == 2 and fig["edge_pairs"] == 3 and abs(fig["zone_ms"]["block_first31_moving"] - 0.045) < 1e-12 and abs(fig["zone_ms"]["block_first31"] - 0.03) < 1e-12
    assert abs(fig["peak"] - 0.3) < 1e-12 and abs(fig["peak_clean"] - 0.1) < 1e-12
    bars = {"peak": 1.0, "peak_clean": 0.2, "ratio": {}, "zone": {"block_first31": 100.0}, "zone_ms": {"block_first31_moving": 0.05}}
    assert not S.violations("lmr", fig, bars)
    assert [v[1] for v in S.violations("lmr", fig, dict(bars, peak_clean=0.05, zone_ms={"block_first31_moving": 0.04}))] == ["peak_clean", "zone_ms:block_first31_moving"]
    k, m, c, ed = S.kept_pairs(np.array([[0.0, 0.001, 0.02, 0.02, 0.02]]), np.array([[0.0, 0.0, 0.02, 0.02, 0.02]]))
    assert k.tolist() == [[True, True, False, True, True]] and m.tolist() == [[False, False, False, True, False]] and c.tolist() == [[True, False, False, False, True]] and ed.tolist() == [[True, True, False, False, True]]


def test_without_a_defect_every_ratio_stays_near_one(surrogate):
    """White noise, N samples pooled a position, P positions: E2[p] / sigma^2 is chi-square(N dof) / N, standard deviation sqrt(2 / N) (complex
    samples and stereo frames: sqrt(1 / N)), and the largest of P lies about sqrt(2 ln P) of them above 1.  Seen here (8 stations x 26 blocks):
    every worst-position and zone ratio between 0.99 and 1.25 for the plain surrogate, between 0.97 and 1.26 for the one scaled by the local level
    (the 1.25: the four-tile fold of L+R, 208-416 samples a position, 1024 positions).  Asserted: the worst position within 1 + 6 (plain) or 1 + 9
    (scaled: the level's fourth moment widens it) standard deviations, zones of |Z| positions within 12 / sqrt(|Z|) of them + 0.1."""
    kind_of, errs = surrogate
    k_sd = 6.0 if kind_of == "plain" else 9.0
    seen = []
    for k in S.STREAMS:
        fig = S.figures(errs[k], GEO[k])
        n = S.squared(errs[k]).shape[2]
        for kind, r in fig["ratio"].items():
            if r is None:
                continue
            pooled = N_ST * NB * (n // GEO[k]["periods"][kind.replace("_detrended", "")])
            sd = np.sqrt((1.0 if k in ("fm_out_iq", "audio") else 2.0) / pooled)
            seen.append(r)
            assert 1.0 <= r <= 1.0 + k_sd * sd, (k, kind, r, sd)
        for name, kind, lo, hi in GEO[k]["zones"]:
            pooled = N_ST * NB * (n // GEO[k]["periods"][kind])
            sd = np.sqrt(2.0 / pooled / (hi - lo))
            seen.append(fig["zone"][name])
            assert abs(fig["zone"][name] - 1.0) <= 2 * k_sd * sd + 0.1, (k, name, fig["zone"][name], sd)      # (+ 0.1: the median of P noisy positions sits below their mean)
    print(kind_of, "ratios without a defect: %.3f .. %.3f" % (min(seen), max(seen)))


def passes_todays_bars(k, e, oracle_run):
    """The existing checks of test_gpu_fast._compare on a defected error array: whole-run RMS for lpr / fm_out_iq / pll_dt, lmr_audio_excess for L-R / audio."""
    if k == "fm_out_iq":
        return rms(np.stack([e.real, e.imag], axis=-1)) <= S.RMS_BAR[k]
    if k in ("lpr", "pll_dt"):
        return rms(e) <= S.RMS_BAR[k]
    for c, o in enumerate(oracle_run):
        g = {j: [None] * c + [o[j].reshape(-1).astype(np.float64)] for j in ("lmr", "audio", "lmr_phase")}
        g[k][c] = g[k][c] + e[c].reshape(-1)
        if lmr_audio_excess(g, o, c, NB)[0] > 1.0:
            return False
    return True


def test_every_defect_is_flagged_and_still_passes_todays_rms_bars(surrogate, oracle_run):
    """The defects today's bars let through — A / 4 once per period at position 0, T / 2, T - 1 (A = B sqrt(T)); B sqrt(block / |Z|) / 4 over the
    block's first 31 outputs and first span — fail the bars of test_gpu_fast_seams.py, while each defected array passes rms / lmr_audio_excess."""
    kind_of, errs = surrogate
    # the ratio and zone bars alone: white noise over a million samples peaks at 5-6 sigma by construction (the GPU's pll_dt error is a slow
    # drift that peaks at 3), so the peak bars are left out here and every defect has to be caught BY POSITION
    bars = {k: dict(BARS[k], peak=np.inf) for k in S.STREAMS}
    misses, smallest, zones = sensitivity(errs, GEO, None, bars)
    print(kind_of, "smallest caught multiple of A:", smallest, zones)
    assert not misses, misses
    assert all(v for z in zones.values() for v in z.values()), zones
    for k in S.STREAMS:
        assert not S.violations(k, S.figures(errs[k], GEO[k]), bars[k]), (k, "the surrogate itself must pass")
        n = S.squared(errs[k]).shape[2]
        for kind, t in GEO[k]["periods"].items():
            if t >= n:
                continue
            for pos in (0, t // 2, t - 1):
                assert passes_todays_bars(k, S.inject(errs[k], t, S.RMS_BAR[k] * np.sqrt(t) / 4, pos), oracle_run), (k, kind, pos)
        if k != "fm_out_iq":
            lo, hi = (0, 128) if k == "pll_dt" else (0, 31)
            assert passes_todays_bars(k, S.inject(errs[k], n, S.RMS_BAR[k] * np.sqrt(n / (hi - lo)) / 4, lo, hi), oracle_run), (k, "zone")
