"""Band scanner, host side (no GPU): the default FFT size and detection parameters, the detection rules of fmd_scan_detect against their
float64 restatement (tests/scan_ref.py) on numpy PSDs of synthetic captures and on hand-made corner cases, planted stations found
exactly, and the refusals."""
import math

import numpy as np
import pytest

from scan_ref import DEFAULTS, plant, ref_detect, ref_psd


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


def _same(pkg, psd, fs_in, **params):
    got = pkg.scan_detect(psd, fs_in, **params)
    ref = ref_detect(psd, fs_in, **params)
    assert list(got["offset_hz"]) == [r[0] for r in ref]
    for g, r in zip(got, ref):
        assert abs(g["power_db"] - r[1]) <= 1e-9
        assert (g["snr_db"] == r[2]) if math.isinf(r[2]) else abs(g["snr_db"] - r[2]) <= 1e-9
    return got


@pytest.mark.parametrize("fs_in,nfft", [(1_024_000.0, 256), (10_000_000.0, 2048), (20_480_000.0, 4096), (32_768_000.0, 8192),
                                        (250_000.0, 256), (100e6, 16384), (5_000_000.0, 1024)])
def test_default_nfft(pkg, fs_in, nfft):
    assert pkg.scan_default_nfft(fs_in) == nfft
    assert pkg.load_library().fmd_scan_default_nfft(fs_in) == nfft


def test_default_params(pkg):
    assert pkg.scan_default_params() == DEFAULTS


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_detection_matches_the_restatement_on_synthetic_captures(pkg, seed):
    """about 4 MSa/s, stations at random raster points and levels, the PSD by numpy; also with other parameters"""
    rng = np.random.default_rng(seed)
    fs_in = 4_096_000.0
    pts = rng.choice(np.arange(-15, 16), size=5, replace=False) * 100e3
    stations = [(float(f), float(rng.uniform(8, 40)), k) for k, f in enumerate(pts)]
    x = plant(120_000, fs_in, stations, seed=seed)
    psd, frames = ref_psd(x, pkg.scan_default_nfft(fs_in), fs_in)
    assert frames > 100
    _same(pkg, psd, fs_in)
    _same(pkg, psd, fs_in, raster_hz=50e3, min_spacing_hz=120e3, min_snr_db=6.0)
    _same(pkg, psd, fs_in, raster_hz=200e3, raster_origin_hz=100e3, channel_bw_hz=150e3, usable_fraction=0.6, noise_quantile=0.3)
    _same(pkg, psd, fs_in, min_spacing_hz=0.0)


def _flat(n=1024, level=1.0):
    return np.full(n, level)


def test_raster_origin(pkg):
    fs_in, n = 1_024_000.0, 1024                      # bin width 1 kHz
    psd = _flat(n)
    psd[n // 2 + 25 - 3:n // 2 + 25 + 4] = 1e4        # energy around +25 kHz
    assert list(_same(pkg, psd, fs_in, raster_hz=50e3, raster_origin_hz=25e3, channel_bw_hz=20e3)["offset_hz"]) == [25e3]
    assert list(_same(pkg, psd, fs_in, raster_hz=50e3, channel_bw_hz=20e3)["offset_hz"]) == []


def test_usable_band_edge(pkg):
    """a raster point whose channel ends exactly on the usable edge is scanned; one a bin further out is not"""
    fs_in, n = 1_024_000.0, 1024
    lim = 0.8 * fs_in / 2                              # 409.6 kHz
    psd = _flat(n)
    psd[n // 2 + 350:n // 2 + 360] = 1e3               # +350 kHz: its 100 kHz channel ends at 400 kHz <= 409.6 kHz
    psd[n // 2 - 405] = 1e5                            # -405 kHz: usable, but in no channel (-400 kHz's would end at -450 kHz)
    got = _same(pkg, psd, fs_in, raster_hz=50e3, min_spacing_hz=100e3)
    assert list(got["offset_hz"]) == [350e3]
    got = _same(pkg, psd, fs_in, raster_hz=50e3, min_spacing_hz=100e3, usable_fraction=400e3 / (fs_in / 2))   # edge exactly at 400 kHz
    assert list(got["offset_hz"]) == [350e3]
    assert lim > 400e3


def test_whole_band_usable_channel_ends_at_nyquist(pkg):
    """usable_fraction = 1 with a 50 kHz raster: the raster points at +-4.95 MHz of 10 MSa/s have channels that end exactly at +-fs_in / 2.
    The window stops at the last bin (+fs_in / 2 is bin N, which does not exist: it is bin 0, -fs_in / 2)."""
    fs_in, n = 10_000_000.0, 2048                      # bin width 4882.8125 Hz
    psd = _flat(n)
    psd[n - 3:] = 1e3                                  # the top three bins, up to +fs_in / 2 - one bin
    psd[:3] = 1e3                                      # the bottom three, from -fs_in / 2
    got = _same(pkg, psd, fs_in, raster_hz=50e3, usable_fraction=1.0)
    assert list(got["offset_hz"]) == [-4.95e6, 4.95e6]
    top = ref_detect(psd, fs_in, raster_hz=50e3, usable_fraction=1.0)[1]
    hi_bins = n - 1 - (math.ceil((4.9e6) / (fs_in / n)) + n // 2) + 1                  # bins from 4.9 MHz up to bin N - 1
    assert abs(top[1] - 10 * math.log10(fs_in / n * (3e3 + hi_bins - 3))) < 1e-9
    assert abs(top[2] - 10 * math.log10((3e3 + hi_bins - 3) / hi_bins)) < 1e-9   # n_c counts only the bins that exist
    # the same through the C ABI with a PSD buffer of exactly N doubles and nothing after it
    import ctypes as C
    buf = (C.c_double * n)(*psd)
    out = np.zeros(8, pkg.SCAN_STATION_DTYPE)
    cnt = C.c_int(0)
    p = pkg.capi._scan_params(dict(raster_hz=50e3, usable_fraction=1.0))
    assert pkg.load_library().fmd_scan_detect(buf, n, fs_in, C.byref(p), out.ctypes.data_as(C.c_void_p), 8, C.byref(cnt)) == 0
    assert cnt.value == 2 and list(out["offset_hz"][:2]) == [-4.95e6, 4.95e6]


def test_raster_too_fine_is_refused(pkg):
    for r in (1e-300, 5e-324, 1e-3):
        with pytest.raises(pkg.FmdError, match="raster points"):
            pkg.scan_detect(_flat(1024), 1_024_000.0, raster_hz=r)
    assert len(pkg.scan_detect(_flat(1024), 1_024_000.0, raster_hz=1.0, min_spacing_hz=0.0)) == 0   # 819201 points: allowed


def test_tie_break_takes_the_lower_offset(pkg):
    fs_in, n = 1_024_000.0, 1024
    psd = _flat(n)
    psd[n // 2 - 100] = psd[n // 2 + 0] = 1e4          # equal power at -100 and 0 kHz, 100 kHz apart
    got = _same(pkg, psd, fs_in)
    assert list(got["offset_hz"]) == [-100e3]


def test_zero_noise_floor(pkg):
    fs_in, n = 1_024_000.0, 1024
    psd = np.zeros(n)
    psd[n // 2 + 200] = 1e-20
    got = _same(pkg, psd, fs_in)
    assert list(got["offset_hz"]) == [200e3] and math.isinf(got["snr_db"][0]) and got["snr_db"][0] > 0
    assert len(pkg.scan_detect(np.zeros(n), fs_in)) == 0        # P_c = 0 is never reported


def test_capacity_smaller_than_the_count(pkg):
    import ctypes as C
    fs_in, n = 1_024_000.0, 1024
    psd = _flat(n)
    for f in (-300, -100, 100, 300):
        psd[n // 2 + f] = 1e4
    lib = pkg.load_library()
    out = np.zeros(3, pkg.SCAN_STATION_DTYPE)
    out["offset_hz"] = 7.0
    cnt = C.c_int(-1)
    p = pkg.capi._scan_params({})
    rc = lib.fmd_scan_detect(psd.ctypes.data_as(C.c_void_p), n, fs_in, C.byref(p), out.ctypes.data_as(C.c_void_p), 2, C.byref(cnt))
    assert rc == 0 and cnt.value == 4
    assert list(out["offset_hz"]) == [-300e3, -100e3, 7.0]
    rc = lib.fmd_scan_detect(psd.ctypes.data_as(C.c_void_p), n, fs_in, C.byref(p), None, 0, C.byref(cnt))
    assert rc == 0 and cnt.value == 4
    assert list(pkg.scan_detect(psd, fs_in)["offset_hz"]) == [-300e3, -100e3, 100e3, 300e3]


def test_planted_strong_station_is_reported_once(pkg):
    fs_in = 4_096_000.0
    x = plant(200_000, fs_in, [(300e3, 40.0, 0)], seed=11)
    psd, _ = ref_psd(x, pkg.scan_default_nfft(fs_in), fs_in)
    got = _same(pkg, psd, fs_in)
    assert list(got["offset_hz"]) == [300e3]
    assert got["snr_db"][0] > 35


def test_planted_weak_station_beside_a_strong_one(pkg):
    fs_in = 4_096_000.0
    x = plant(200_000, fs_in, [(-500e3, 40.0, 1), (-300e3, 15.0, 2)], seed=12)
    psd, _ = ref_psd(x, pkg.scan_default_nfft(fs_in), fs_in)
    got = _same(pkg, psd, fs_in)
    assert list(got["offset_hz"]) == [-500e3, -300e3]


@pytest.mark.parametrize("bad,match", [
    (dict(raster_hz=0.0), "raster_hz"), (dict(raster_hz=-1.0), "raster_hz"), (dict(channel_bw_hz=0.0), "channel_bw_hz"),
    (dict(usable_fraction=0.0), "usable_fraction"), (dict(usable_fraction=1.5), "usable_fraction"),
    (dict(noise_quantile=-0.1), "noise_quantile"), (dict(noise_quantile=1.01), "noise_quantile"),
    (dict(min_spacing_hz=-1.0), "min_spacing_hz"), (dict(min_snr_db=float("nan")), "min_snr_db"),
    (dict(raster_origin_hz=float("inf")), "raster_origin_hz"),
])
def test_bad_parameters_are_refused_with_a_message(pkg, bad, match):
    with pytest.raises(pkg.FmdError, match=match):
        pkg.scan_detect(_flat(256), 1_024_000.0, **bad)


def test_bad_psd_nfft_and_rate_are_refused(pkg):
    psd = _flat(256)
    with pytest.raises(pkg.FmdError, match="power of two"):
        pkg.scan_detect(_flat(300), 1_024_000.0)
    with pytest.raises(pkg.FmdError, match="power of two"):
        pkg.scan_detect(_flat(128), 1_024_000.0)
    with pytest.raises(pkg.FmdError, match="power of two"):
        pkg.scan_detect(_flat(32768), 1_024_000.0)
    with pytest.raises(pkg.FmdError, match="fs_in"):
        pkg.scan_detect(psd, 0.0)
    with pytest.raises(pkg.FmdError, match="fs_in"):
        pkg.scan_detect(psd, -1e6)
    bad = psd.copy()
    bad[17] = np.nan
    with pytest.raises(pkg.FmdError, match="not finite"):
        pkg.scan_detect(bad, 1_024_000.0)
    bad[17] = np.inf
    with pytest.raises(pkg.FmdError, match="not finite"):
        pkg.scan_detect(bad, 1_024_000.0)
    with pytest.raises(pkg.FmdError):
        pkg.scan_default_nfft(0.0)
    with pytest.raises(TypeError):
        pkg.scan_detect(psd, 1_024_000.0, raster=1.0)


def test_bad_scanner_configurations_are_refused(pkg):
    """refused before any device is touched, so this holds without a GPU"""
    for kw, match in ((dict(fs_in=0.0), "fs_in"), (dict(fs_in=-5.0), "fs_in"), (dict(fs_in=10e6, nfft=1000), "power of two"),
                      (dict(fs_in=10e6, nfft=128), "power of two"), (dict(fs_in=10e6, nfft=32768), "power of two"),
                      (dict(fs_in=10e6, max_input_samples=0), "max_input_samples")):
        with pytest.raises(pkg.FmdError, match=match):
            pkg.BandScanner(**kw)


def test_symbols_are_declared_in_the_product_header(pkg):
    names = set(pkg.declared_symbols(debug=False))
    for s in ("fmd_scan_default_nfft", "fmd_scan_default_params", "fmd_scan_detect", "fmd_scan_create", "fmd_scan_destroy", "fmd_scan_reset",
              "fmd_scan_process_cf32_dev", "fmd_scan_process_u8_dev", "fmd_scan_process_s8_dev", "fmd_scan_process_s16_dev",
              "fmd_scan_get_psd", "fmd_scan_stations", "fmd_scan_last_error"):
        assert s in names
        assert hasattr(pkg.load_library(), s)
