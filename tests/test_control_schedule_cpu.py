"""The blockwise oracle driver of tests/control_schedules.py against oraclelib.run_chain (CPU only): stepping the oracle block by block
through a schedule of control events gives run_chain's bits where run_chain can express the same run — no events, or events that all fall
on block 0 — with the coefficient override (as the GPU tests drive it) and without it (the oracle's own update_filters designs)."""
import numpy as np
import pytest

import control_schedules as S
import oraclelib as O
import synth
from conftest import bits_equal, describe_diff

BS, NB, FS = 8192, 4, 256_000
STREAMS = ["fm_out_iq", "pll_dt", "lpr", "lmr", "rds", "rds_raw_sym", "rds_sym", "audio", "lmr_phase"]
BLOCK0 = dict(use_deemphasis=1, deemphasis_tus=75, lpr_cutoff_hz=9000, lmr_cutoff_hz=12000, audio_stereo_mix_factor=0.65)


@pytest.fixture(scope="module")
def caps():
    return np.stack([synth.to_cf32(synth.fm_capture(NB * BS, fs=float(FS), seed=31, channel=c)["iq"]) for c in range(2)])


def _same(res, want, c):
    for k in STREAMS:
        assert bits_equal(S.joined(res, k, c), want[k]), f"station {c} {k}: {describe_diff(S.joined(res, k, c), want[k])}"
    assert np.array_equal(S.joined(res, "rds_count", c), want["rds_count"])
    assert np.array_equal(S.joined(res, "rds_bytes", c), want["rds_bytes"])


def _ctl(fields):
    c = O.default_controls()
    for k, v in fields.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("override", [False, True])
def test_empty_schedule_equals_run_chain(caps, override):
    k = O.design(FS)
    res = S.run_oracle(caps, BS, FS, [], coeffs=[[k, k]] * NB if override else None, streams=STREAMS)
    for c in range(2):
        _same(res, O.run_chain(caps[c], BS, FS, u8=False, coeffs=k if override else None, streams=STREAMS), c)


@pytest.mark.parametrize("override", [False, True])
def test_events_on_block_0_equal_run_chain_with_controls(caps, override):
    """Station 1 gets its controls in two events before block 0 (the second on top of the first); station 0 stays at the defaults."""
    first = {k: BLOCK0[k] for k in ("use_deemphasis", "deemphasis_tus", "lpr_cutoff_hz")}
    rest = {k: v for k, v in BLOCK0.items() if k not in first}
    sched = [(0, 1, first), (0, 1, rest)]
    ks = [O.design(FS), O.design(FS, _ctl(BLOCK0))]
    res = S.run_oracle(caps, BS, FS, sched, coeffs=[ks] * NB if override else None, streams=STREAMS)
    for c, ctl in ((0, None), (1, _ctl(BLOCK0))):
        _same(res, O.run_chain(caps[c], BS, FS, u8=False, controls=ctl, coeffs=ks[c] if override else None, streams=STREAMS), c)


def test_timeline_and_reference_arguments():
    calls, force = S.timeline(S.S5, S.N_STATIONS, S.N_BLOCKS)
    assert force[1][1] == S.defaults() and force[2][1]["lpr_cutoff_hz"] == 12000 and len(calls[2]) == 2
    assert all(f["use_deemphasis"] == 1 and f["lmr_cutoff_hz"] == 12000 and f["lpr_cutoff_hz"] == 15000 for f in force[4])     # channel -1: defaults + fields
    assert force[5][2]["use_deemphasis"] == 0 and force[5][2]["deemphasis_tus"] == 50 and force[5][3]["use_deemphasis"] == 1
    assert S.touched(S.S1, 6) == {1, 2, 4} and S.touched(S.S5, 6) == set(range(6))
    assert S.ref_args(S.station_schedule(S.S3, 2)) == ["deemph=on", "tus=50", "at=5", "tus=75"]
    assert S.ref_args(S.station_schedule(S.S1, 4)) == ["at=7", "lpr=11000", "lmr=7000"]
