"""Whole-band channeliser on the GPU: capture rates of 16 - 32.768 MSa/s -> 256 kSa/s stations (the whole FM band in one capture).
Same definition as tests/test_channelizer.py, same float64 restatement as the oracle.  Which kernel serves a configuration:
  * L dividing 16 and the band form's tile within its LDS budget (16, 20, 20.48, 24, 30.72, 32, 32.768 MSa/s with the default taps):
    k_channelize_band_mfma, on the matrix cores, with a tile of G = 8 or 4 groups of 16 outputs (G = 2 with 3000 taps per phase at
    32.768 MSa/s);
  * every other pair beyond the 128-output window (25 MSa/s: L = 32; 20 MSa/s with 4096 taps per phase, whose prototype would not fit the
    band form's LDS): k_channelize with a tile of fewer outputs.
Every case asserts the form its handle reports (Channelizer.form, Channelizer.tile_outputs).
"""
import os

import numpy as np
import pytest

import synth
from rds_groups import decode_groups
from test_channelizer import ref_channelize

FS_OUT = 256_000.0
# fs_in -> (L, M, default taps per phase)
RATES = {
    16_000_000.0: (2, 125, 1024),
    20_000_000.0: (8, 625, 1280),
    20_480_000.0: (1, 80, 1312),
    24_000_000.0: (4, 375, 1536),
    25_000_000.0: (32, 3125, 1600),
    30_720_000.0: (1, 120, 1968),
    32_000_000.0: (1, 125, 2048),
    32_768_000.0: (1, 128, 2100),
}
# (fs_in, taps per phase, form)
FORMS = [(f, 0, "k_channelize_band_mfma") for f in RATES if f != 25e6] + [
    (25e6, 0, "k_channelize, tile of 32"),
    (20e6, 4096, "k_channelize, tile of 32 (L = 8 divides 16; the 128 KB prototype exceeds the band form's LDS)"),
    (32.768e6, 3000, "k_channelize_band_mfma"),          # G = 2: the 3000-tap prototype leaves room for two groups' rails
]
# (fs_in, taps per phase) -> Channelizer.tile_outputs: the band form's 16 G (G = 8, 4 or 2 groups), k_channelize's tile
TILES = {(16e6, 0): 128, (20.48e6, 0): 128, (20e6, 0): 64, (24e6, 0): 64, (30.72e6, 0): 64, (32e6, 0): 64, (32.768e6, 0): 64,
         (32.768e6, 3000): 32, (25e6, 0): 32, (20e6, 4096): 32}
# white noise against the float64 definition, max|y - ref| / max|ref| over the whole output: twice the worst figure measured on an MI355X
# over FORMS (2.41e-6, at 20.48 MSa/s; DESIGN.md §6 "Tap placement"), in place of the 2e-5 the test had
NOISE_BAR = 4.9e-6

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    return p


def _cf(y):
    y = y.cpu().numpy() if hasattr(y, "cpu") else y
    return y[..., 0] + 1j * y[..., 1]


def _input(rng, n_in):
    x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
    return x


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.float32).reshape(-1, 2)).cuda()


def test_whole_band_rates_are_accepted(pkg):
    for fs_in, (L, M, T) in RATES.items():
        ch = pkg.Channelizer(fs_in, [0.0, 0.3 * fs_in], max_input_samples=M * 64)
        assert (ch.interp, ch.decim, ch.taps_per_phase) == (L, M, T), fs_in
        ch.close()


def test_limits_are_refused_with_a_message(pkg):
    with pytest.raises(pkg.FmdError, match="M / L <= 128"):
        pkg.Channelizer(40e6, [0.0], max_input_samples=625 * 16, taps_per_phase=2048)        # M / L = 156.25
    with pytest.raises(pkg.FmdError, match="4096"):
        pkg.Channelizer(20.48e6, [0.0], max_input_samples=80 * 16, taps_per_phase=4100)


@pytest.mark.parametrize("fs_in,tpp,form", FORMS)
def test_matches_the_float64_definition(pkg, fs_in, tpp, form):
    import torch
    rng = np.random.default_rng(int(fs_in) // 1000 + tpp)
    L, M = RATES[fs_in][:2]
    n_out = L * -(-650 // L)                              # 40 groups of 16 and a part of one
    n_in = n_out * M // L
    x = _input(rng, n_in)
    centers = np.linspace(-0.45, 0.45, 6) * fs_in + 1234.5
    ch = pkg.Channelizer(fs_in, centers, max_input_samples=n_in, taps_per_phase=tpp)
    assert form.startswith(ch.form + ",") or form == ch.form, (form, ch.form)
    assert ch.tile_outputs == TILES[fs_in, tpp], form
    y = _cf(ch.process(_dev(torch, x)))
    assert y.shape == (6, n_out)
    taps = ch.taps()
    worst = 0.0
    for k, f in enumerate(centers):
        ref = ref_channelize(x, f, taps, L, M, fs_in=fs_in)
        worst = max(worst, float(np.abs(y[k] - ref).max() / np.abs(ref).max()))
    print(f"{fs_in / 1e6} MSa/s, T = {ch.taps_per_phase}, {form}: max|y - ref| / max|ref| = {worst:.2e}")
    assert worst < NOISE_BAR, (form, worst)
    ch.close()


@pytest.mark.parametrize("fs_in", [20.48e6, 24e6, 25e6])
def test_streaming_uneven_and_shortest_calls(pkg, fs_in):
    """One call == uneven cuts == the shortest legal calls (M inputs -> L outputs: at 20.48 MSa/s ONE output a call, so calls start
    inside a group of 16) alternating over two streams into output buffers with spare capacity, nothing written past n_out."""
    import torch
    rng = np.random.default_rng(7)
    L, M = RATES[fs_in][:2]
    n_out = L * -(-300 // L)
    n_in = n_out * M // L
    x = _input(rng, n_in)
    centers = np.array([-0.41, -0.1, 0.0, 0.07, 0.33, 0.449]) * fs_in
    ch = pkg.Channelizer(fs_in, centers, max_input_samples=n_in)
    xt = _dev(torch, x)
    y = _cf(ch.process(xt))
    scale = np.abs(y).max()
    unit, nu = M, n_in // M
    for cuts in ([0, 3 * unit, 4 * unit, (nu // 2) * unit, n_in], [0, (nu - 1) * unit, n_in]):
        ch.reset()
        ys = _cf(torch.cat([ch.process(xt[a:b].contiguous()).clone() for a, b in zip(cuts[:-1], cuts[1:])], dim=1))
        assert ys.shape == y.shape
        assert np.abs(ys - y).max() <= 5e-6 * scale, cuts
    ch.reset()
    bigs = [torch.full((6, L + 7, 2), 7.0, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for i in range(n_in // unit):
        st = streams[i & 1]
        with torch.cuda.stream(st):
            big = bigs[i & 1]
            got = ch.process(xt[i * unit:(i + 1) * unit].contiguous(), out=big, stream=st.cuda_stream)
            assert tuple(got.shape) == (6, L, 2)
            outs.append(got.clone())
            assert float(big[:, L:].min()) == 7.0 and float(big[:, L:].max()) == 7.0
    torch.cuda.synchronize()
    y3 = _cf(torch.cat(outs, dim=1))
    assert np.abs(y3 - y).max() <= 5e-6 * scale
    ch.close()


@pytest.mark.parametrize("fs_in", [20.48e6, 25e6])
def test_station_output_does_not_depend_on_row_or_batch(pkg, fs_in):
    """The same centre in row 0 of a 1-station handle, row 57 of a 100-station handle and the last row of a 256-station handle: bit for bit."""
    import torch
    rng = np.random.default_rng(11)
    L, M = RATES[fs_in][:2]
    n_out = L * -(-400 // L)
    n_in = n_out * M // L
    xt = _dev(torch, _input(rng, n_in))
    f0 = 3.217e6
    got = []
    for n_st, row in ((1, 0), (100, 57), (256, 255)):
        centers = rng.uniform(-0.45, 0.45, n_st) * fs_in
        centers[row] = f0
        ch = pkg.Channelizer(fs_in, centers, max_input_samples=n_in)
        got.append(ch.process(xt)[row].cpu().numpy().copy())
        ch.close()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def test_tone_isolation_at_whole_band_density(pkg):
    """100 stations on the 200 kHz raster across 20.48 MSa/s, a tone 30 kHz off one of them: unit power there, >= 50 dB down elsewhere."""
    import torch
    fs_in = 20.48e6
    n_in = 80 * 2048
    centers = (np.arange(100) - 49.5) * 200e3
    ch = pkg.Channelizer(fs_in, centers, max_input_samples=n_in)
    k0 = 61
    n = np.arange(n_in)
    x = np.exp(2j * np.pi * (((centers[k0] + 30e3) / fs_in * n) % 1.0)).astype(np.complex64)
    y = ch.process(_dev(torch, x)).cpu().numpy()
    p = (y[..., 0].astype(np.float64) ** 2 + y[..., 1].astype(np.float64) ** 2)[:, 256:].mean(axis=1)
    assert abs(p[k0] - 1.0) < 1e-3, p[k0]
    assert np.delete(p, k0).max() < 1e-5, np.delete(p, k0).max()
    ch.close()


FS_E2E = 20.48e6


def _band_station(args):
    """(worker process) one station of the whole-band capture: its 256 kSa/s FM signal resampled to 20.48 MSa/s and shifted to its centre"""
    k, n_out, n_in, center = args
    from scipy.signal import resample_poly
    st = synth.fm_capture(n_out, fs=FS_OUT, seed=700 + k, channel=k)
    up = resample_poly(st["iq"].astype(np.complex128), 80, 1)[:n_in]
    n = np.arange(n_in, dtype=np.float64)
    return (up * np.exp(2j * np.pi * ((center / FS_E2E * n) % 1.0))).astype(np.complex64)


_WIDE = None


def _band_reference(args):
    """(worker process) the float64 restatement of the channeliser for one station (scipy upfirdn with the library's taps)"""
    center, hflat, interp, decim, n_out = args
    from scipy.signal import upfirdn
    wide = _WIDE
    n = np.arange(wide.size, dtype=np.float64)
    xm = wide.astype(np.complex128) * np.exp(-2j * np.pi * ((center / FS_E2E * n) % 1.0))
    y = upfirdn(hflat, xm, interp, decim)[:n_out]
    return np.stack([y.real, y.imag], axis=-1).astype(np.float32)


def test_whole_band_capture_through_channeliser_and_demodulator(pkg):
    """16 FM stations, each with its own RDS PI code, in one 20.48 MSa/s capture spread over +-10 MHz (one of them 240 kHz from +fs_in / 2)
    -> k_channelize_band_mfma -> the batched demodulator in the tolerance mode.  Every station's audio against the same demodulator fed
    the float64-channelised station: <= 1e-4 RMS behind the start-up; every PI code decoded."""
    from concurrent.futures import ProcessPoolExecutor

    import torch
    n_st, bs, nb = 16, 16384, 10
    n_out = bs * nb
    n_in = n_out * 80
    centers = np.linspace(-9.9e6, 10.0e6, n_st)
    assert FS_E2E / 2 - centers[-1] <= 250e3
    workers = min(n_st, 16, max(1, os.cpu_count() or 1))
    with ProcessPoolExecutor(workers) as ex:
        wide = None
        for part in ex.map(_band_station, [(k, n_out, n_in, centers[k]) for k in range(n_st)]):
            wide = part.astype(np.complex128) if wide is None else wide + part
    wide = (wide / n_st).astype(np.complex64)
    ch = pkg.Channelizer(FS_E2E, centers, max_input_samples=bs * 80)
    hflat = ch.taps().astype(np.float64).reshape(-1)
    global _WIDE
    _WIDE = wide
    with ProcessPoolExecutor(workers) as ex:
        ref = np.stack(list(ex.map(_band_reference, [(centers[k], hflat, ch.interp, ch.decim, n_out) for k in range(n_st)])))
    _WIDE = None
    dm = pkg.BatchDemod(n_st, bs, int(FS_OUT), fast_math=True)
    direct = pkg.BatchDemod(n_st, bs, int(FS_OUT), fast_math=True)
    wt = _dev(torch, wide)
    audio, audio_direct, rds_bytes = [], [], [[] for _ in range(n_st)]
    step = bs * 80
    for b in range(nb):
        y = ch.process(wt[b * step:(b + 1) * step].contiguous())
        assert tuple(y.shape) == (n_st, bs, 2)
        dm.process(y.contiguous())
        audio.append(dm.audio())
        byt, cnt = dm.rds_bytes()
        for k in range(n_st):
            rds_bytes[k].append(bytes(byt[k, :cnt[k]]))
        direct.process(np.ascontiguousarray(ref[:, b * bs:(b + 1) * bs]))
        audio_direct.append(direct.audio())
    a, ad = np.concatenate(audio, axis=1), np.concatenate(audio_direct, axis=1)
    errs = [float(np.sqrt(np.mean((a[k, 4096:].astype(np.float64) - ad[k, 4096:]) ** 2))) for k in range(n_st)]
    pis_ok = [k for k in range(n_st) if (0x1234 + k) in {g[0] for g in decode_groups(np.frombuffer(b"".join(rds_bytes[k]), np.uint8))}]
    print(f"whole band end to end, 16 stations at 20.48 MSa/s: audio vs float64-channelised worst {max(errs):.2e} median {np.median(errs):.2e}; "
          f"PI codes decoded {len(pis_ok)} / {n_st}")
    assert max(errs) <= 1e-4, errs
    assert len(pis_ok) == n_st, pis_ok
    ch.close(); dm.close(); direct.close()
