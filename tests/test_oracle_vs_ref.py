"""The oracle against the compiled reference itself (oracle/_ref/fm_ref_dump).

Where the _ref binaries exist (built from the reference's sources by `make -C oracle ref`), live: every stream the
reference exposes must be bit-identical to the restatement on the same input.  Elsewhere against the reference's
outputs on the same inputs, recorded as digests in tests/golden/ref_records.json (tests/golden/make_ref_records.py):
the same bit-identity, stream by stream.
"""
import hashlib

import numpy as np
import pytest

import oraclelib as O
import synth
from conftest import bits_equal, describe_diff

STREAMS = ["fm_out_iq", "pilot", "pll", "pll_raw_err", "pll_pi_err", "lpr", "lmr", "lmr_phase", "rds", "rds_raw_sym", "rds_sym",
           "audio", "bpsk_pll_sym", "bpsk_intdump", "bpsk_ted_raw", "bpsk_ted_pi", "bpsk_pll_raw", "bpsk_pll_pi"]
BOOL_TRACES = ("bpsk_zcd", "bpsk_trig")   # the reference's two bool traces (bpsk_synchroniser.h:79-80); the oracle hands them out as 0 / 1 floats

CHAIN_CASES = [(65536, 24), (16384, 40), (8192, 24), (131072, 8)]
CONTROL_CASES = [
    (["deemph=50"], dict(use_deemphasis=1, deemphasis_tus=50)),
    (["deemph=75", "audio=lmr"], dict(use_deemphasis=1, deemphasis_tus=75, audio_out=1)),
    (["audio=lpr", "lpr=12000"], dict(audio_out=0, lpr_cutoff_hz=12000)),
    (["mix=0.65", "lmr=9000", "lpr=100"], dict(audio_stereo_mix_factor=0.65, lmr_cutoff_hz=9000, lpr_cutoff_hz=100)),
    (["lpr=70000", "deemph=100"], dict(lpr_cutoff_hz=70000, use_deemphasis=1, deemphasis_tus=100)),
]


def chain_capture() -> np.ndarray:
    return synth.to_u8(synth.fm_capture(24 * 65536, seed=2024)["iq"])


def cf32_capture() -> np.ndarray:
    return synth.to_cf32(synth.fm_capture(6 * 65536, seed=77)["iq"])


def noise_capture() -> np.ndarray:
    rng = np.random.default_rng(3)
    return np.clip(np.rint(127 + 30 * rng.standard_normal((4 * 65536, 2))), 0, 255).astype(np.uint8)


def chain_key(block_size, n_blocks) -> str:
    return f"oracle_vs_ref/chain/{block_size}x{n_blocks}"


def controls_key(args) -> str:
    return "oracle_vs_ref/controls/" + " ".join(args)


def digests(streams: dict) -> dict:
    """The reference's (or the oracle's) streams as digests, in the form the live comparison compares them."""
    d = {k: O.digest(streams[k]) for k in STREAMS + ["rds_count", "rds_bytes"]}
    d.update({k: O.digest(np.asarray(streams[k]).astype(np.float32)) for k in BOOL_TRACES})
    return d


def capture_sha256(cap: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(cap).tobytes()).hexdigest()


def _assert_same(ref, orc):
    for k in STREAMS:
        assert bits_equal(ref[k], orc[k]), f"{k}: {describe_diff(ref[k], orc[k])}"
    assert np.array_equal(ref["rds_count"], orc["rds_count"])
    for k in BOOL_TRACES:
        assert np.array_equal(ref[k].astype(np.float32), orc[k]), k
    assert np.array_equal(ref["rds_bytes"], orc["rds_bytes"])


def _check(key, cap, orc, tmp_path, live=None, **ref_kw):
    """The oracle's streams `orc` for capture `cap` against the reference: live where oracle/_ref exists (`live`: and can run the case), else as recorded."""
    if O.have_ref() if live is None else live:
        _assert_same(O.run_ref_chain(cap, tmp_path, **ref_kw), orc)
        return
    rec = O.ref_records()[key]
    if capture_sha256(cap) != rec["capture_sha256"]:
        pytest.skip("synthetic capture not bit-reproducible with this numpy build")
    mine = digests(orc)
    bad = [k for k in rec["streams"] if mine[k] != rec["streams"][k]]
    assert set(mine) == set(rec["streams"]) and not bad, f"streams that differ from the reference's recorded outputs: {bad}"


@pytest.fixture(scope="module")
def capture_u8():
    return chain_capture()


@pytest.mark.parametrize("block_size,n_blocks", CHAIN_CASES)
def test_chain_bit_exact(tmp_path, capture_u8, block_size, n_blocks):
    cap = capture_u8[: block_size * n_blocks]
    _check(chain_key(block_size, n_blocks), cap, O.run_chain(cap, block_size), tmp_path, block_size=block_size)


def _ctl(**kw):
    c = O.default_controls()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("args,ctl", CONTROL_CASES)
def test_controls_bit_exact(tmp_path, capture_u8, args, ctl):
    cap = capture_u8[: 65536 * 6]
    _check(controls_key(args), cap, O.run_chain(cap, 65536, controls=_ctl(**ctl)), tmp_path, block_size=65536, extra_args=args)


def schedule_cases():
    """(name, one-station schedule, cf32?): every station that S1-S4 (tests/control_schedules.py) touch, as a run of its own, and one cf32 run."""
    import control_schedules as S
    cases = []
    for name in ("S1", "S2", "S3", "S4", "S4b"):
        for st in sorted(S.touched(S.SCHEDULES[name], S.N_STATIONS)):
            one = S.station_schedule(S.SCHEDULES[name], st)
            if name == "S4b" and one == S.station_schedule(S.S4, st):
                continue
            cases.append((f"{name}/station{st}", one, False))
    cases.append(("S3/station0/cf32", S.station_schedule(S.S3, 0), True))
    return cases


def schedule_key(name) -> str:
    return "oracle_vs_ref/schedule/" + name


def schedule_capture(cf32: bool) -> np.ndarray:
    return cf32_capture()[: 16384 * 12] if cf32 else chain_capture()[: 16384 * 12]


def flat(res: dict) -> dict:
    """The blockwise driver's one-station result in run_chain's form."""
    import control_schedules as S
    return {k: S.joined(res, k, 0) for k in res}


@pytest.mark.parametrize("name,sched,cf32", schedule_cases(), ids=[c[0] for c in schedule_cases()])
def test_control_schedule_bit_exact(tmp_path, name, sched, cf32):
    """Controls changed between blocks: a filter re-designed under a live history, a de-emphasis IIR whose state stays frozen while
    it is switched off, the mixing switched from one block to the next (reference UpdateFilters, broadcast_fm_demod.cpp:330-389, and
    the switch at :404): twelve 16384-sample blocks, the reference given the events as at=<block> arguments (oracle/ref_dump.cpp).
    An fm_ref_dump kept from before the harness took those arguments cannot run the case: then, as without oracle/_ref, the recorded digests decide."""
    import control_schedules as S
    cap = schedule_capture(cf32)
    orc = flat(S.run_oracle(cap[None], 16384, 1_024_000, sched, streams=STREAMS + list(BOOL_TRACES)))
    _check(schedule_key(name), cap, orc, tmp_path, live=O.ref_takes_schedules(), block_size=16384, u8=not cf32, extra_args=S.ref_args(sched))


def test_cf32_boundary_bit_exact(tmp_path):
    cap = cf32_capture()
    _check("oracle_vs_ref/cf32", cap, O.run_chain(cap, 65536, u8=False), tmp_path, block_size=65536, u8=False)


def test_noise_only_input_bit_exact(tmp_path):
    """No station: PLLs never lock, AGC rails — exercises the unlocked/acquisition dynamics."""
    cap = noise_capture()
    _check("oracle_vs_ref/noise", cap, O.run_chain(cap, 65536), tmp_path, block_size=65536)
