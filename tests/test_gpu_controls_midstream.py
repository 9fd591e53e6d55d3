"""GPU tests (pytest -m gpu) of control changes BETWEEN blocks, per station, against the CPU oracle (tests/control_schedules.py).

fmd_set_controls is the demodulator's only run-time input besides the samples.  What it leaves behind — the per-station tap rows, the
tolerance mode's table of tap images per distinct cut-off and the per-station index into it, the fact that switches k_extract_bp<2> on and
off, the de-emphasis state machine (none / inside the front tile / the serial stage, which lingers for one block after the last station
leaves it) and the drain in front of the re-upload — is what every stage of a block goes by.  The oracle takes the same events block by
block; tests/test_oracle_vs_ref.py::test_control_schedule_bit_exact pins it to the compiled reference under the same schedules.

Exact mode: every stream of gpu_parity.STREAMS, the RDS symbols, counts and bytes bit-identical to the oracle in EVERY block, the block of
a change and the one behind it included; a station without an event bit-identical to the same handle shape run without any event; the
same through a device tensor, through fmd_submit_*, without the pipeline, and across fmd_reset.

Tolerance mode: every block and station within the mode's bars of the oracle (TOL_RMS on the discriminator output and L+R,
test_gpu_fast.lmr_audio_excess on L-R and audio, the RDS bits once in lock).  ONE exclusion: the in-tile de-emphasis has no state (it
starts from zero 128 samples early), the oracle's IIR starts or resumes from the state it froze with; in a block in which a station's
filter is switched on or off or changes its time constant the first 32 audio samples (1 ms; 128 of fm_out_iq) are left out of the RMS
and bound instead by the peak, over that window, of the oracle's own difference between that station run with the filter always on and
always off.  The windows are under 1 % of any station's stream (asserted).  Cut-off and mixing changes get the plain bars on the change
block too: both sides apply the new taps to the same history.  So does a station that filters on unchanged while the handle changes
between the in-tile form and the serial stage: the in-tile form hands its last sample to the serial stage as its state.  (Before it
did, the serial stage started from whatever it last held: station 2 of T1, 50 -> 150 us at block 4, missed the L+R bar of that block
OUTSIDE the window with 3.5e-4 RMS, and station 0, 75 us throughout, was 2.9e-2 off inside it.)
"""
import ctypes as C

import numpy as np
import pytest

import control_schedules as S
import oraclelib as O
import synth
from conftest import rms
from gpu_parity import STREAMS, lib_coeffs_to_oracle
from test_gpu_fast import TOL_RMS, lmr_audio_excess, record_parity_metrics, same_bits_once_in_lock

pytestmark = pytest.mark.gpu

KEYS = STREAMS + S.EXTRA
# rate -> fs, block of the exact-mode runs (the smallest made of whole 1024-output front tiles), u8
RATES = {"256k": (256_000, 8192, False), "1024k": (1_024_000, 16384, True)}
SCHEDULES = dict(S.SCHEDULES, S5=S.S5)


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    import torch
    assert torch.cuda.is_available()
    return p


_cache = {}


def _caps(n_ch, n, fs, seed, u8=False):
    key = ("caps", n_ch, n, fs, seed, u8)
    if key not in _cache:
        conv = synth.to_u8 if u8 else synth.to_cf32
        _cache[key] = np.stack([conv(synth.fm_capture(n, fs=float(fs), seed=seed, channel=c)["iq"]) for c in range(n_ch)])
        _cache[key].setflags(write=False)
    return _cache[key]


def _exact_caps(rate):
    fs, bs, u8 = RATES[rate]
    return _caps(S.N_STATIONS, S.N_BLOCKS * bs, fs, seed=8100, u8=u8)


def _exact_run(pkg, name, rate):
    """The exact mode's run of a schedule through process (numpy), computed once (name None: no events)."""
    key = ("exact", name, rate)
    if key not in _cache:
        fs, bs, _ = RATES[rate]
        _cache[key] = S.run_gpu(pkg, _exact_caps(rate), bs, fs, SCHEDULES[name] if name else [])
    return _cache[key]


def _assert_no_differences(a, b, stations, what, **kw):
    bad = S.differences(a, b, stations, keys=KEYS, **kw)
    assert not bad, f"{what}: {len(bad)} (station, stream, block) differ, first {bad[:6]}"


# ---- exact mode --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", list(RATES))
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_exact_mode_schedule_is_bit_identical_to_the_oracle_in_every_block(pkg, name, rate):
    fs, bs, _ = RATES[rate]
    caps, sched = _exact_caps(rate), SCHEDULES[name]
    g = _exact_run(pkg, name, rate)
    o = S.run_oracle(caps, bs, fs, sched, coeffs=g["coeffs"])
    _assert_no_differences(g, o, range(S.N_STATIONS), f"{name} {rate} against the oracle")
    # a station the schedule never touches: the drain and the re-upload must not be visible to it
    untouched = sorted(set(range(S.N_STATIONS)) - S.touched(sched, S.N_STATIONS))
    assert untouched or name == "S5"
    _assert_no_differences(g, _exact_run(pkg, None, rate), untouched, f"{name} {rate}: untouched stations against a run without events")


@pytest.mark.parametrize("form", ["torch", "submit", "unpipelined"])
@pytest.mark.parametrize("name", ["S3", "S4", "S4b"])
def test_exact_mode_schedule_through_the_other_entry_points(pkg, name, form):
    """The de-emphasis schedules through a device tensor, through fmd_submit_* (every drain cuts the pilot PLL's hand-over chain) and
    without the pipeline: what process (numpy) gives, which the test above holds to the oracle."""
    fs, bs, _ = RATES["256k"]
    kw = dict(pipelined=False) if form == "unpipelined" else dict(entry=form)
    g = S.run_gpu(pkg, _exact_caps("256k"), bs, fs, SCHEDULES[name], **kw)
    _assert_no_differences(g, _exact_run(pkg, name, "256k"), range(S.N_STATIONS), f"{name} through {form}")


def test_exact_mode_reset_in_the_middle_of_a_schedule(pkg):
    """fmd_reset behind S3's block 5 (two stations filtering, one switched off with a frozen state, one about to switch on): the six
    blocks behind it are those of a fresh handle given the controls in force at the reset and the schedule's later events."""
    fs, bs, _ = RATES["256k"]
    caps = _exact_caps("256k")
    g = S.run_gpu(pkg, caps, bs, fs, S.S3, reset_after=5)
    _, in_force = S.timeline(S.S3, S.N_STATIONS, S.N_BLOCKS)
    fresh_sched = [(0, c, in_force[5][c]) for c in range(S.N_STATIONS)] + [(b - 6, st, f) for b, st, f in S.S3 if b >= 6]
    fresh = S.run_gpu(pkg, caps[:, 6 * bs:], bs, fs, fresh_sched)
    behind = {k: [blocks[6:] for blocks in g[k]] for k in KEYS}
    _assert_no_differences(behind, fresh, range(S.N_STATIONS), "blocks behind the reset against a fresh handle")
    _assert_no_differences(g, _exact_run(pkg, "S3", "256k"), range(S.N_STATIONS), "blocks in front of the reset", blocks=range(6))


# ---- tolerance mode ----------------------------------------------------------------------------------------------------------------

FAST_BLOCKS = 24
WINDOW = 32                 # audio samples (1 ms): the library's own figure (fmd_api.cpp upload_controls); x 4 of fm_out_iq
# the de-emphasis schedules with every station's last de-emphasis event inside the first 0.3 s (blocks 0-4 of 64 ms), so that the
# RDS comparison has 1.2 s behind it
FAST_SCHEDULES = {
    "S1": S.S1, "S2": S.S2,
    "S3": S.remapped(S.S3, {0: 0, 2: 1, 3: 1, 4: 2, 5: 2, 6: 3, 7: 4, 8: 4}),
    "S4": S.remapped(S.S4, {0: 0, 3: 1, 5: 2, 6: 3, 7: 4}),
    "S4b": S.remapped(S.S4B, {0: 0, 3: 1, 5: 2, 7: 4}),
}
# T1: station 2 leaves what the in-tile form covers at block 4 (the handle falls back to the serial stage) and returns at block 8;
# station 0 filters throughout and sees both changes of form
T1 = [(0, 0, dict(use_deemphasis=1, deemphasis_tus=75)), (0, 2, dict(use_deemphasis=1, deemphasis_tus=50)),
      (4, 2, dict(deemphasis_tus=150)), (8, 2, dict(deemphasis_tus=50))]


def windows(sched, n_ch, nb):
    """{(block, station)}: where the one exclusion applies — the station's own filter is switched on or off or changes its time constant
    (not block 0: both sides start from zero there).  A station that filters on unchanged while the HANDLE changes between the in-tile form
    and the serial stage gets no window: the in-tile form leaves its last sample as the serial stage's state (k_front_mfma)."""
    _, force = S.timeline(sched, n_ch, nb)
    out = set()
    for b in range(1, nb):
        for c in range(n_ch):
            was, now = force[b - 1][c], force[b][c]
            if was["use_deemphasis"] != now["use_deemphasis"] or (now["use_deemphasis"] and was["deemphasis_tus"] != now["deemphasis_tus"]):
                out.add((b, c))
    return out


def _window_bound(cap, bs, fs, u8, force, coeffs, b):
    """Peak, over block b's window, of the oracle's own difference between the station run with the filter always on and always off
    (the block's other controls in force from the start), per stream."""
    runs = []
    for use in (1, 0):
        ctl = S._fill(O.Controls(), {**force, "use_deemphasis": use})
        runs.append(O.run_chain(cap[: (b + 1) * bs], bs, fs, u8=u8, controls=ctl, coeffs=lib_coeffs_to_oracle(coeffs), streams=["fm_out_iq", "lpr", "lmr", "audio"]))
    out = {}
    for k, per in _per_block(bs, fs).items():
        w = WINDOW * per // _per_block(bs, fs)["lpr"]
        d = np.abs(runs[0][k].astype(np.float64) - runs[1][k]).reshape(b + 1, per)[b, :w]
        out[k] = float(d.max())
    return out


def _per_block(bs, fs):
    n_audio = bs // (fs // 256_000) // 2 // 4
    return {"fm_out_iq": 8 * n_audio, "lpr": n_audio, "lmr": n_audio, "audio": 2 * n_audio}


def hold_to_the_oracle(g, caps, bs, fs, sched, rds_skip_bits, what):
    """The tolerance mode's bars for run g of `sched`, every block and station; -> the measured figures."""
    n_ch, nb = caps.shape[0], caps.shape[1] // bs
    u8 = caps.dtype == np.uint8
    o = S.run_oracle(caps, bs, fs, sched, coeffs=g["coeffs"], streams=["fm_out_iq", "lpr", "lmr", "audio", "lmr_phase"])
    _, force = S.timeline(sched, n_ch, nb)
    win = windows(sched, n_ch, nb)
    per = _per_block(bs, fs)
    figures = {"worst_rms": {k: 0.0 for k in ("fm_out_iq", "lpr")}, "lmr_audio_excess": 0.0, "windows": len(win), "window_peak": {}, "window_bound": {}}
    for c in range(n_ch):
        mine = sorted(b for b, st in win if st == c)
        share = len(mine) * WINDOW / (nb * per["lpr"])
        assert share < 0.01, (what, c, share)
        gj = {k: S.joined(g, k, c).astype(np.float64).reshape(nb, -1) for k in per}
        oj = {k: S.joined(o, k, c).astype(np.float64).reshape(nb, -1) for k in per}
        for b in mine:
            bound = _window_bound(caps[c], bs, fs, u8, force[b][c], g["coeffs"][b][c], b)
            for k in per:
                w = WINDOW * per[k] // per["lpr"]
                err = gj[k][b] - oj[k][b]
                peak = float(np.max(np.abs(err[:w])))
                figures["window_peak"][f"{k}/station{c}/block{b}"] = peak
                figures["window_bound"][f"{k}/station{c}/block{b}"] = bound[k]
                print(f"{what} window station {c} block {b} {k}: peak {peak:.3e} bound {bound[k]:.3e}")
                assert peak <= bound[k], (what, c, b, k, peak, bound[k])
                # out of the RMS: the window takes the RMS of the block's other samples, so the block's RMS is theirs
                gj[k][b, :w] = oj[k][b, :w] + rms(err[w:])
        for k in ("fm_out_iq", "lpr"):
            e = np.sqrt(((gj[k] - oj[k]) ** 2).mean(axis=1))
            figures["worst_rms"][k] = max(figures["worst_rms"][k], float(e.max()))
            assert e.max() <= TOL_RMS, (what, c, k, int(e.argmax()), float(e.max()))
        gm = {"lmr": [gj["lmr"].reshape(-1)] * (c + 1), "audio": [gj["audio"].reshape(-1)] * (c + 1), "lmr_phase": [S.joined(g, "lmr_phase", c)] * (c + 1)}
        om = {"lmr": oj["lmr"].reshape(-1), "audio": oj["audio"].reshape(-1), "lmr_phase": S.joined(o, "lmr_phase", c)}
        ex = lmr_audio_excess(gm, om, c, nb)[0]
        figures["lmr_audio_excess"] = max(figures["lmr_audio_excess"], ex)
        assert ex <= 1.0, (what, c, ex)
        assert same_bits_once_in_lock(S.joined(g, "rds_bytes", c), S.joined(o, "rds_bytes", c), skip_bits=rds_skip_bits), (what, c)
    print(what, {k: v for k, v in figures.items() if not isinstance(v, dict)}, figures["worst_rms"])
    record_parity_metrics(f"controls_midstream/{what}", figures)
    return figures


def _skip_bits(sched):
    """The skips test_gpu_fast uses: 12 x 76 bits where a station de-emphasises, else 5 x 76."""
    return (12 if any("use_deemphasis" in f for _, _, f in sched) else 5) * 76


FAST_STREAMS = ["fm_out_iq", "lpr", "lmr", "audio", "lmr_phase"]


@pytest.mark.parametrize("name", list(FAST_SCHEDULES))
def test_tolerance_mode_schedule_is_within_the_bars_around_every_change(pkg, name):
    fs, bs = 256_000, 16384
    caps = _caps(S.N_STATIONS, FAST_BLOCKS * bs, fs, seed=8200)
    g = S.run_gpu(pkg, caps, bs, fs, FAST_SCHEDULES[name], fast_math=True, streams=FAST_STREAMS)
    hold_to_the_oracle(g, caps, bs, fs, FAST_SCHEDULES[name], _skip_bits(FAST_SCHEDULES[name]), f"{name}_256k_cf32")


def test_tolerance_mode_de_emphasis_schedule_at_1024k_u8(pkg):
    """S3 in 32 ms blocks of u8 samples (48 blocks = 1.5 s), where the front end is k_predecim_mfma + k_front_mfma while a station filters."""
    fs, bs = 1_024_000, 32768
    caps = _caps(S.N_STATIONS, 48 * bs, fs, seed=8201, u8=True)
    g = S.run_gpu(pkg, caps, bs, fs, FAST_SCHEDULES["S3"], fast_math=True, streams=FAST_STREAMS)
    hold_to_the_oracle(g, caps, bs, fs, FAST_SCHEDULES["S3"], 12 * 76, "S3_1024k_u8")


# ... and with nobody filtering in front of block 2 and behind block 10: at 1.024 MSa/s the front end is k_front_pre_mfma there, the two
# kernels in between (fmd_plan.h front_takes_capture), in the in-tile form, on the serial stage and in the in-tile form again
T1_PRE = [(2, 0, dict(use_deemphasis=1, deemphasis_tus=75)), (2, 2, dict(use_deemphasis=1, deemphasis_tus=50)),
          (4, 2, dict(deemphasis_tus=150)), (8, 2, dict(deemphasis_tus=50)), (10, 0, S.OFF), (10, 2, S.OFF)]


@pytest.mark.parametrize("fs,bs,u8,nb,name", [(256_000, 16384, False, FAST_BLOCKS, "T1"), (1_024_000, 32768, True, 48, "T1"), (1_024_000, 32768, True, 48, "T1_pre")])
def test_tolerance_mode_change_between_the_in_tile_form_and_the_serial_stage(pkg, fs, bs, u8, nb, name):
    """T1.  Station 2 goes from 50 to 150 us at block 4 — beyond what the in-tile form covers, so the whole handle falls back to the
    serial k_deemphasis stage, which continues from the state the in-tile form left — and back at block 8.  Station 0 filters at 75 us
    throughout and has no window: it is held to the plain bars through both changes of form."""
    caps = _caps(S.N_STATIONS, nb * bs, fs, seed=8201 if u8 else 8200, u8=u8)
    sched = T1 if name == "T1" else T1_PRE
    assert windows(sched, S.N_STATIONS, nb) == ({(4, 2), (8, 2)} if name == "T1" else {(2, 0), (2, 2), (4, 2), (8, 2), (10, 0), (10, 2)})
    g = S.run_gpu(pkg, caps, bs, fs, sched, fast_math=True, streams=FAST_STREAMS)
    hold_to_the_oracle(g, caps, bs, fs, sched, 12 * 76, f"{name}_{fs // 1000}k")


def test_tolerance_mode_table_of_tap_images_grows_under_way(pkg):
    """T2.  Eleven stations; at each of blocks 1-10 one more station gets a pair of cut-offs no station had (the values of
    test_fast_mode_odd_block_length_and_per_station_cut_offs), so the table of tap images per distinct cut-off passes its first allocation
    of 8 slots at block 4 and every station's index is uploaded again ten times.  Every station is held to the oracle, and until its own
    change a station is bit-identical to a run without events."""
    fs, bs, n_ch = 256_000, 16384, 11
    caps = _caps(n_ch, FAST_BLOCKS * bs, fs, seed=8203)
    sched = [(c, c, dict(lpr_cutoff_hz=15000 - 700 * c, lmr_cutoff_hz=14000 - 600 * c)) for c in range(1, n_ch)]
    g = S.run_gpu(pkg, caps, bs, fs, sched, fast_math=True, streams=FAST_STREAMS)
    hold_to_the_oracle(g, caps, bs, fs, sched, 5 * 76, "T2_table_growth")
    plain = S.run_gpu(pkg, caps, bs, fs, [], fast_math=True, streams=FAST_STREAMS)
    for c in range(n_ch):
        bad = S.differences(g, plain, [c], keys=FAST_STREAMS + S.EXTRA, blocks=range(c if c else FAST_BLOCKS))
        assert not bad, (c, bad[:4])


@pytest.mark.parametrize("n_ch", [6, 7])
@pytest.mark.parametrize("case", ["cut-offs", "serial stage"])
def test_tolerance_mode_pairing_follows_the_controls(pkg, case, n_ch):
    """T3.  k_extract_bp<2> wherever possible (set_extract_pairing(1)): it runs while the cut-offs are uniform and the handle is not on the
    serial de-emphasis stage... and whatever it does, every output is bit-identical to one station per workgroup (mode 2)."""
    fs, bs, nb = 256_000, 16384, 12
    caps = _caps(n_ch, nb * bs, fs, seed=8204)
    if case == "cut-offs":
        sched = [(4, 3, dict(lpr_cutoff_hz=9000, lmr_cutoff_hz=12000)), (8, 3, dict(lpr_cutoff_hz=15000, lmr_cutoff_hz=15000))]
    else:
        sched = [(0, 1, dict(use_deemphasis=1, deemphasis_tus=50)), (4, 1, dict(deemphasis_tus=150)), (8, 1, dict(deemphasis_tus=50))]
    a = S.run_gpu(pkg, caps, bs, fs, sched, fast_math=True, streams=FAST_STREAMS, pairing=1)
    b = S.run_gpu(pkg, caps, bs, fs, sched, fast_math=True, streams=FAST_STREAMS, pairing=2)
    bad = S.differences(a, b, range(n_ch), keys=FAST_STREAMS + S.EXTRA)
    assert not bad, (len(bad), bad[:6])


def _rds_symbol_tensors(dm):
    """Zero-copy views of fmd_rds_dev's buffers (the block the device-side output calls refer to): (symbols [C, n_rds], counts [C])."""
    import torch
    ps, pc = C.c_void_p(), C.c_void_p()
    dm._check(dm.L.fmd_rds_dev(dm.h, C.byref(ps), C.byref(pc)))
    n_ch, n_rds = dm.n_channels, dm.rates.n_rds

    class _S:
        __cuda_array_interface__ = {"shape": (n_ch * n_rds,), "typestr": "<f4", "data": (ps.value, False), "version": 2}

    class _N:
        __cuda_array_interface__ = {"shape": (n_ch,), "typestr": "<i4", "data": (pc.value, False), "version": 2}
    return torch.as_tensor(_S(), device="cuda").view(n_ch, n_rds), torch.as_tensor(_N(), device="cuda")


def test_tolerance_mode_put_off_extract_stage_keeps_its_block_s_controls(pkg):
    """T4.  1024 stations x 16384 samples at 256 kSa/s: the smallest batch on the deferred schedule (fmd_plan.h kLazyMinSamples), where
    fmd_submit_* puts block k's extract stage off until block k + 1's front end is queued.  Controls set between the two submissions must
    reach block k + 1 only: the drain queues the put-off stage with the old tables before they are rewritten.  S1's events and a
    de-emphasis switch at block 4, on the first station, the last, and the second of a pair; read with fmd_set_output_lag(1) as
    test_submit_schedule_and_output_lag_in_the_tolerance_mode reads; audio, symbols and bytes of every block against the same schedule
    through process (which tests above hold to the oracle on six stations)."""
    import torch
    from fm_radio_amd.capi import Controls
    fs, bs, nb, n_ch = 256_000, 16384, 8, 1024
    where = {1: 0, 2: 513, 4: n_ch - 1}
    sched = [(b, where[st], f) for b, st, f in S.S1] + [(4, st, dict(use_deemphasis=1, deemphasis_tus=50)) for st in where.values()]
    calls, _ = S.timeline(sched, n_ch, nb)
    base = torch.from_numpy(_caps(8, nb * bs, fs, seed=8205).copy()).cuda()
    idx = torch.from_numpy(np.arange(n_ch) % 8).cuda()
    blocks = [base[:, b * bs:(b + 1) * bs][idx].contiguous() for b in range(nb)]

    def host_outputs(dm):
        sy, cn = dm.rds_symbols()
        by, bc = dm.rds_bytes()
        return dm.audio().copy(), sy.copy(), cn.copy(), by.copy(), bc.copy()

    def set_block_controls(dm, b):
        for st, full in calls[b]:
            dm.set_controls(S._fill(Controls(), full), st)

    ref = pkg.BatchDemod(n_ch, bs, fs, fast_math=True)
    want = []
    for b in range(nb):
        set_block_controls(ref, b)
        assert ref.process(blocks[b]) == 0
        want.append(host_outputs(ref))
    ref.close()
    # the events are visible where they should be: the changed stations differ from their twins (same capture, no event) from the change on
    for b, st in ((3, 0), (3, 513), (4, n_ch - 1)):
        twin = st + 8 if st + 8 < n_ch else st - 8
        assert np.array_equal(want[b - 1][0][st], want[b - 1][0][twin]) and not np.array_equal(want[b][0][st], want[b][0][twin]), (b, st)

    dm = pkg.BatchDemod(n_ch, bs, fs, fast_math=True)
    dm.set_output_lag(True)
    side = torch.cuda.Stream()
    kept = {}
    for b in range(nb):
        set_block_controls(dm, b)
        assert dm.submit(blocks[b]) == 0
        with torch.cuda.stream(side):
            dm.wait_outputs(side)
            k = dm.outputs_block()
            assert k == b - 1, (b, k)
            if k >= 0:
                sy, cn = _rds_symbol_tensors(dm)
                by, bc = dm.rds_bytes_tensors()
                kept[k] = (dm.audio_tensor().clone(), sy.clone(), cn.clone(), by.clone(), bc.clone())
                dm.release_outputs(side)
    dm.synchronize(); side.synchronize()
    got = {k: tuple(t.cpu().numpy() for t in v) for k, v in kept.items()}
    got[nb - 1] = host_outputs(dm)
    dm.close()
    for b in range(nb):
        audio, sy, cn, by, bc = got[b]
        w_audio, w_sy, w_cn, w_by, w_bc = want[b]
        bad = np.nonzero((audio.reshape(n_ch, -1).view(np.uint32) != w_audio.reshape(n_ch, -1).view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, f"block {b}: audio of {bad.size} stations differs, first {bad[:8]}"
        assert np.array_equal(cn, w_cn) and np.array_equal(bc, w_bc), b
        for c in range(n_ch):
            assert np.array_equal(sy[c, :cn[c]].view(np.uint32), w_sy[c, :cn[c]].view(np.uint32)), (b, c)
            assert np.array_equal(by[c, :bc[c]], w_by[c, :bc[c]]), (b, c)
