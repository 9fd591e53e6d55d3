"""Whole-band channeliser rates, host side (no GPU): the default taps per phase (fmd_chan_default_taps_per_phase) and the prototype
they give meeting the channeliser's filter specification at every whole-band rate a receiver of the FM band delivers."""
import numpy as np
import pytest

FS_OUT = 256_000.0
# fs_in -> (L, M, default taps per phase): 640 where fmd_chan_create has always accepted it, else the 64 us of capture 640 taps span at 10 MSa/s
RATES = {
    10_000_000.0: (16, 625, 640),
    12_800_000.0: (1, 50, 640),
    16_000_000.0: (2, 125, 1024),
    20_000_000.0: (8, 625, 1280),
    20_480_000.0: (1, 80, 1312),
    24_000_000.0: (4, 375, 1536),
    25_000_000.0: (32, 3125, 1600),
    30_720_000.0: (1, 120, 1968),
    32_000_000.0: (1, 125, 2048),
    32_768_000.0: (1, 128, 2100),
}
WHOLE_BAND = [f for f in RATES if f >= 16e6]


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


@pytest.mark.parametrize("fs_in", list(RATES))
def test_default_taps_per_phase(pkg, fs_in):
    L, M, T = RATES[fs_in]
    assert pkg.chan_default_taps(fs_in, FS_OUT) == T
    assert pkg.load_library().fmd_chan_default_taps_per_phase(fs_in, FS_OUT) == T
    _, l, m = pkg.chan_design(fs_in, FS_OUT, T)
    assert (l, m) == (L, M)


def test_default_taps_keep_640_wherever_it_was_accepted(pkg):
    """Every pair with 128 M / L + 642 <= 7168 keeps 640 taps per phase, so no configuration that worked before changes."""
    for fs_in in np.arange(256_000, 14_000_001, 64_000, dtype=np.int64):
        _, L, M = pkg.chan_design(float(fs_in), FS_OUT, 4)
        t = pkg.chan_default_taps(float(fs_in), FS_OUT)
        if 128 * M // L + 642 <= 7168:
            assert t == 640, fs_in
        else:
            assert t == 4 * -(-512 * M // (125 * L)), fs_in


def test_default_taps_refuse_what_the_designer_refuses(pkg):
    assert pkg.load_library().fmd_chan_default_taps_per_phase(10e6, 256e3 + 0.5) < 0
    with pytest.raises(pkg.FmdError):
        pkg.chan_default_taps(10e6, 0.0)


@pytest.mark.parametrize("fs_in", WHOLE_BAND)
def test_whole_band_prototype_meets_the_specification(pkg, fs_in):
    """Same specification as tests/test_channelizer.py at 10 MSa/s: +-100 kHz flat to 0.1 dB, >= 55 dB down from 156 kHz up to
    fs_in / 2 (everything there aliases into the station)."""
    T = pkg.chan_default_taps(fs_in, FS_OUT)
    taps, L, M = pkg.chan_design(fs_in, FS_OUT, T)
    h = taps.astype(np.float64).reshape(-1)              # [t][p] flattened == prototype order n = t L + p
    fs_up = L * fs_in
    f = np.concatenate([np.linspace(0, 100e3, 41), np.linspace(156e3, fs_in / 2, 1200)])
    H = np.abs(np.exp(-2j * np.pi * np.outer(f / fs_up, np.arange(h.size))) @ h) / L
    assert np.all(np.abs(20 * np.log10(H[:41])) < 0.1)
    assert np.all(20 * np.log10(H[41:]) < -55.0)
    assert abs(h.sum() - L) < 1e-3
