"""The channeliser's tap placement, pinned exactly on every kernel form (plan and checkers: tests/chan_impulse.py; their preconditions:
tests/test_chan_impulse_cpu.py).  A train of M impulses, T + 1 or a few more samples apart, shows every one of the L T prototype taps in
exactly one output and leaves every other output zero.  At the centres 0 and +-fs_in / 4 the output must EQUAL the library's own tap
times the impulse's amplitude and (-j)^(+-n_i), value for value, on every form, format, batch size and cut of the input into calls:
a dropped or misplaced edge tap, an off-by-one in a band's structural zero, a wrong sample at a K-slice or call boundary each change
at least one output from a tap to zero or to another tap.  At three generic centres per handle the bound is per output and relative
to that output's own tap (chan_impulse.B_GENERIC: the mixer's fp32 phasor).  Every configuration asserts the kernel form it runs."""
import numpy as np
import pytest

import chan_impulse as CI

pytestmark = pytest.mark.gpu

SHAPES = ("one", "shortest", "uneven")


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    return p


def _handle(pkg, cfg, plan_fmt="cf32", center_hz=None):
    """(handle, plan, device capture) of a configuration, the handle's form asserted against the configuration's label"""
    import torch
    fs_in, tpp, form, tile = cfg
    cs = CI.centers(fs_in) if center_hz is None else center_hz
    T = tpp or pkg.chan_default_taps(fs_in, CI.FS_OUT)
    _, L, M = pkg.chan_design(fs_in, CI.FS_OUT, 4)
    plan = CI.ImpulsePlan(L, M, T, plan_fmt)
    ch = pkg.Channelizer(fs_in, cs, max_input_samples=plan.n_in, taps_per_phase=tpp)
    assert (ch.interp, ch.decim, ch.taps_per_phase) == (L, M, T)
    assert (ch.form, ch.tile_outputs) == (form, tile), (CI.config_id(cfg), ch.form, ch.tile_outputs)
    return ch, plan, torch.from_numpy(plan.input()).cuda()


def _run(ch, xt, cuts):
    """the stream in the calls `cuts` gives, on a reset handle: [C, n_out, 2] float32 on the host"""
    import torch
    ch.reset()
    outs = [ch.process(xt[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return (outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)).cpu().numpy()


def _check_six_rows(ch, plan, fs_in, y, label):
    """rows 0-2 against the exact expectation, rows 3-5 within the bound: the worst ratio of the generic rows"""
    taps = ch.taps()
    assert y.shape == (6, plan.n_out, 2)
    for k, q in enumerate(CI.QUARTERS):
        CI.check_exact(y[k], plan.expected_exact(taps, q))
    worst = 0.0
    for k in range(3, 6):
        ref, scale = plan.expected_float64(taps, ch.centers[k], fs_in)
        worst = max(worst, CI.check_bounded(y[k], ref, scale))
    print(f"{label}: generic centres, worst |y - ref| / (|h| |a|) = {worst:.2e}")
    return worst


def _assert_sensitive(ch, plan, fs_in, y):
    """the checkers on the GPU's own (passing) output: the smallest edge tap zeroed, and the stream shifted by one output, are rejected"""
    taps = ch.taps()
    first = int(np.flatnonzero(plan.out_tap == 0)[0])
    dropped = y.copy()
    dropped[:, first] = 0
    shifted = np.roll(y, 1, axis=1)
    want = plan.expected_exact(taps, CI.QUARTERS[1])
    ref, scale = plan.expected_float64(taps, ch.centers[3], fs_in)
    assert np.abs(want[first]).max() > 0 and scale[first] > 0
    for bad in (dropped, shifted):
        with pytest.raises(AssertionError):
            CI.check_exact(bad[1], want)
        with pytest.raises(AssertionError):
            CI.check_bounded(bad[3], ref, scale)


@pytest.mark.parametrize("cfg", CI.CONFIGS, ids=CI.config_id)
def test_every_tap_lands_in_its_output(pkg, cfg):
    """cf32, six stations (three exact centres, three generic), in one call, in the shortest legal calls and in uneven ones"""
    ch, plan, xt = _handle(pkg, cfg)
    for shape in SHAPES:
        y = _run(ch, xt, plan.cuts(shape, cfg[3]))
        _check_six_rows(ch, plan, cfg[0], y, f"{CI.config_id(cfg)}, cf32, {shape}")
        if shape == "one":
            _assert_sensitive(ch, plan, cfg[0], y)
    ch.close()


# one configuration of each kernel (the band form with its largest and its smallest tile): the integer staging paths of the matrix-core
# forms are not the cf32 ones
INT_CONFIGS = [c for c in CI.CONFIGS if (c[0], c[1]) in ((10e6, 640), (10e6, 704), (2.4e6, 0), (20.48e6, 0), (32.768e6, 3000))]


@pytest.mark.parametrize("fmt", ["u8", "s16"])
@pytest.mark.parametrize("cfg", INT_CONFIGS, ids=CI.config_id)
def test_every_tap_lands_in_its_output_from_integer_captures(pkg, cfg, fmt):
    ch, plan, xt = _handle(pkg, cfg, fmt)
    for shape in SHAPES:
        y = _run(ch, xt, plan.cuts(shape, cfg[3]))
        _check_six_rows(ch, plan, cfg[0], y, f"{CI.config_id(cfg)}, {fmt}, {shape}")
    ch.close()


@pytest.mark.parametrize("n_st", [7, 300])
def test_every_row_of_a_batch_at_10_msa_s(pkg, n_st):
    """k_channelize16_mfma walks several tiles per workgroup when 512 / C < n_tiles: C = 7 gives 73 workgroups for 81 tiles (some take
    two), C = 300 one workgroup for all 81.  The rows cycle through the three exact centres and every row equals the exact expectation,
    so rows with the same centre are identical across row and batch."""
    cfg = (10e6, 640, "k_channelize16_mfma", 128)
    quarters = [CI.QUARTERS[k % 3] for k in range(n_st)]
    ch, plan, xt = _handle(pkg, cfg, center_hz=np.array(quarters) * (cfg[0] / 4.0))
    n_tiles = -(-plan.n_out // 128)
    assert n_tiles == 81 and max(1, 512 // n_st) == {7: 73, 300: 1}[n_st]
    want = [plan.expected_exact(ch.taps(), q) for q in CI.QUARTERS]
    for shape in ("one", "uneven"):
        y = _run(ch, xt, plan.cuts(shape, 128))
        assert y.shape == (n_st, plan.n_out, 2)
        for k in range(n_st):
            CI.check_exact(y[k], want[k % 3])
    ch.close()
