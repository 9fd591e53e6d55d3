"""The channeliser on a receiver's integer capture: interleaved u8 (RTL-SDR), s8 (HackRF) and s16 (Airspy, SDRplay, USRP sc16) read by
fmd_chan_process_{u8,s8,s16}_dev / Channelizer.process(uint8 | int8 | int16) without a conversion pass.  The contract: a call on integers
writes exactly the bits a cf32 call writes on the converted samples (u8: v - 127, s8 / s16: v), on every kernel form and for every split of
the input into calls, in any mix of formats.  Which configuration selects which form (fmd_chan_create):
  * 10 MSa/s, 640 taps per phase: k_channelize16_mfma (L = 16 and K = 585 + T <= 1232);
  * 10 MSa/s, 768 taps per phase: k_channelize16 (L = 16, T a multiple of 64, too long for the matrix-core operand);
  * 2.4 MSa/s (L / M = 8 / 75, the RTL-SDR rate): k_channelize;
  * 20.48 and 20 MSa/s: k_channelize_band_mfma with tiles of 8 and 4 groups;
  * 25 MSa/s (L = 32): k_channelize with a tile of 32 outputs.
Every case asserts the form its handle reports (Channelizer.form, Channelizer.tile_outputs).
"""
import os

import numpy as np
import pytest

import synth
from rds_groups import decode_groups
from test_channelizer import ref_channelize

pytestmark = pytest.mark.gpu

FS_OUT = 256_000.0
# (fs_in, taps per phase (0: default), L, M, form)
FORMS = [
    (10e6, 640, 16, 625, "k_channelize16_mfma"),
    (10e6, 768, 16, 625, "k_channelize16"),
    (2.4e6, 0, 8, 75, "k_channelize"),
    (20.48e6, 0, 1, 80, "k_channelize_band_mfma, G = 8"),
    (20e6, 0, 8, 625, "k_channelize_band_mfma, G = 4"),
    (25e6, 0, 32, 3125, "k_channelize, tile of 32"),
]
IDS = [f[4] for f in FORMS]
# what Channelizer.form and Channelizer.tile_outputs must say for each label
KERNELS = {"k_channelize16_mfma": ("k_channelize16_mfma", 128), "k_channelize16": ("k_channelize16", 128), "k_channelize": ("k_channelize", 128),
           "k_channelize_band_mfma, G = 8": ("k_channelize_band_mfma", 128), "k_channelize_band_mfma, G = 4": ("k_channelize_band_mfma", 64),
           "k_channelize, tile of 32": ("k_channelize", 32)}
# integer captures against the float64 definition, max|y - ref| / max|ref| over the whole output: twice the worst figure measured on an
# MI355X over FORMS x FORMATS (3.06e-6, s16 on k_channelize16_mfma; DESIGN.md §6 "Tap placement"), in place of the 2e-5 the test had
NOISE_BAR = 6.2e-6
FORMATS = ("u8", "s8", "s16")
LIMITS = {"u8": (0, 255, np.uint8), "s8": (-128, 127, np.int8), "s16": (-32768, 32767, np.int16)}


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    return p


def _capture(rng, fmt, n):
    """[n, 2] interleaved integers over the type's whole range, its extremes and zero placed at the start, inside and at the end"""
    lo, hi, dt = LIMITS[fmt]
    a = rng.integers(lo, hi + 1, size=(n, 2), endpoint=False).astype(dt)
    special = np.array([[lo, hi], [hi, lo], [0, 0], [lo, lo], [hi, hi], [0, hi]], dt)
    for at in (0, n // 3, n - len(special)):
        a[at:at + len(special)] = special
    return a


def _converted(a):
    """the cf32 samples an integer capture stands for: u8 as the reference converts it, s8 / s16 as their values"""
    return synth.u8_to_cf32(a) if a.dtype == np.uint8 else a.astype(np.float32).reshape(-1, 2)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cf(y):
    y = y.cpu().numpy() if hasattr(y, "cpu") else y
    return y[..., 0].astype(np.float64) + 1j * y[..., 1]


def _sizes(L, M):
    n_out = L * -(-650 // L)                              # 40 groups of 16 and a part of one
    return n_out, n_out * M // L


@pytest.mark.parametrize("fs_in,tpp,L,M,form", FORMS, ids=IDS)
def test_integer_input_is_bit_identical_to_its_cf32_conversion(pkg, fs_in, tpp, L, M, form):
    import torch
    rng = np.random.default_rng(int(fs_in) // 1000 + tpp)
    n_out, n_in = _sizes(L, M)
    centers = np.linspace(-0.45, 0.45, 6) * fs_in + 1234.5
    ch = pkg.Channelizer(fs_in, centers, max_input_samples=n_in, taps_per_phase=tpp)
    assert (ch.interp, ch.decim) == (L, M)
    assert (ch.form, ch.tile_outputs) == KERNELS[form]
    for fmt in FORMATS:
        a = _capture(rng, fmt, n_in)
        ch.reset()
        y_int = ch.process(_dev(torch, a)).clone()
        ch.reset()
        y_f = ch.process(_dev(torch, _converted(a))).clone()
        assert tuple(y_int.shape) == (6, n_out, 2)
        assert torch.equal(y_int, y_f), (form, fmt)
        assert bool(torch.isfinite(y_int).all()) and float(y_int.abs().max()) > 0.0
    ch.close()


@pytest.mark.parametrize("fs_in,tpp,L,M,form", FORMS, ids=IDS)
def test_integer_input_matches_the_float64_definition(pkg, fs_in, tpp, L, M, form):
    """test_channelizer.ref_channelize on the converted samples, with the bound the cf32 tests use"""
    import torch
    rng = np.random.default_rng(int(fs_in) // 1000 + tpp + 1)
    n_out, n_in = _sizes(L, M)
    centers = np.linspace(-0.45, 0.45, 6) * fs_in + 1234.5
    ch = pkg.Channelizer(fs_in, centers, max_input_samples=n_in, taps_per_phase=tpp)
    assert (ch.form, ch.tile_outputs) == KERNELS[form]
    taps = ch.taps()
    for fmt in FORMATS:
        a = _capture(rng, fmt, n_in)
        ch.reset()
        y = _cf(ch.process(_dev(torch, a)))
        xf = _converted(a)
        x = xf[:, 0].astype(np.float64) + 1j * xf[:, 1]
        worst = 0.0
        for k, f in enumerate(centers):
            ref = ref_channelize(x, f, taps, L, M, fs_in=fs_in)
            worst = max(worst, float(np.abs(y[k] - ref).max() / np.abs(ref).max()))
        print(f"{form}, {fmt}: max|y - ref| / max|ref| = {worst:.2e}")
        assert worst < NOISE_BAR, (form, fmt, worst)
    ch.close()


STREAMED = [f for f in FORMS if f[4] in ("k_channelize16_mfma", "k_channelize16", "k_channelize", "k_channelize_band_mfma, G = 8")]


@pytest.mark.parametrize("fs_in,tpp,L,M,form", STREAMED, ids=[f[4] for f in STREAMED])
def test_streamed_calls_in_alternating_formats_over_two_streams(pkg, fs_in, tpp, L, M, form):
    """Uneven legal pieces — among them calls of one unit (fewer samples than the T - 1 of history; at 20.48 MSa/s, L = 1, one output)
    — in the formats u8, cf32, s16, s8 in turn, alternating over two streams: the bits of the same pieces all in cf32.  Each piece's
    samples span its own type's range, so the history a call reads holds samples of other formats."""
    import torch
    rng = np.random.default_rng(5 + tpp)
    unit = M                                              # the shortest legal call: L outputs (one at 20.48 MSa/s)
    units = [3, 1, 70, 1, 1, 5, 2, 1, 190, 4, 1, 6]
    n_in = unit * sum(units)
    ch = pkg.Channelizer(fs_in, np.array([-0.41, -0.1, 0.0, 0.07, 0.33, 0.449]) * fs_in, max_input_samples=n_in, taps_per_phase=tpp)
    assert unit < ch.taps_per_phase - 1 and (ch.form, ch.tile_outputs) == KERNELS[form]
    order = ("u8", "cf32", "s16", "s8")
    pieces, conv = [], []                                 # (format, device tensor) and the piece as cf32
    for i, nu in enumerate(units):
        fmt = order[i % len(order)]
        if fmt == "cf32":
            a = (rng.standard_normal((nu * unit, 2)) * 3000.0).astype(np.float32)
            pieces.append(_dev(torch, a)); conv.append(a)
        else:
            a = _capture(rng, fmt, nu * unit)
            pieces.append(_dev(torch, a)); conv.append(_converted(a))
    conv_dev = [_dev(torch, c) for c in conv]
    whole = _dev(torch, np.concatenate(conv))
    torch.cuda.synchronize()

    def run(inputs):
        ch.reset()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = []
        for i, x in enumerate(inputs):
            st = streams[i & 1]
            with torch.cuda.stream(st):
                outs.append(ch.process(x, stream=st.cuda_stream).clone())
        torch.cuda.synchronize()
        return torch.cat(outs, dim=1)

    mixed = run(pieces)
    all_cf32 = run(conv_dev)
    assert mixed.shape == all_cf32.shape and mixed.shape[1] == n_in * L // M
    assert torch.equal(mixed, all_cf32), form
    ch.reset()
    one = _cf(ch.process(whole))
    assert np.abs(_cf(mixed) - one).max() <= 5e-6 * np.abs(one).max()    # (the cf32 tests' bound between cuts: the mixer's recurrence)
    ch.close()


@pytest.mark.parametrize("fs_in,fmt", [(10e6, "u8"), (20.48e6, "s8"), (25e6, "s16")])
def test_station_output_does_not_depend_on_row_or_batch(pkg, fs_in, fmt):
    """The same centre in row 0 of a 1-station handle, row 57 of a 100-station handle and the last row of a 256-station handle: bit for bit."""
    import torch
    rng = np.random.default_rng(13)
    L, M = {10e6: (16, 625), 20.48e6: (1, 80), 25e6: (32, 3125)}[fs_in]
    n_out = L * -(-400 // L)
    n_in = n_out * M // L
    xt = _dev(torch, _capture(rng, fmt, n_in))
    f0 = 1.217e6
    got = []
    for n_st, row in ((1, 0), (100, 57), (256, 255)):
        centers = rng.uniform(-0.45, 0.45, n_st) * fs_in
        centers[row] = f0
        ch = pkg.Channelizer(fs_in, centers, max_input_samples=n_in)
        got.append(ch.process(xt)[row].clone())
        ch.close()
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


def test_other_dtypes_are_refused_before_the_library(pkg):
    import torch
    ch = pkg.Channelizer(10e6, [0.0], max_input_samples=625 * 4)
    for dt in (torch.float64, torch.int32, torch.float16, torch.bool):
        with pytest.raises(ValueError):
            ch.process(torch.zeros((625, 2), dtype=dt, device="cuda"))
    with pytest.raises(ValueError):
        ch.process(torch.zeros((625, 2), dtype=torch.uint8))                         # host memory
    with pytest.raises(ValueError):
        ch.process(torch.zeros((2, 625), dtype=torch.int16, device="cuda").t())      # not contiguous
    with pytest.raises(pkg.FmdError, match="multiple of 625"):
        ch.process(torch.zeros((1000, 2), dtype=torch.int8, device="cuda"))          # the cf32 path's errors and messages
    ch.close()


def _station(args):
    """(worker process) one station at 256 kSa/s, interpolated to fs_in in stages of short filters (up / down pairs) and shifted to its centre"""
    k, seed, n_out, n_in, fs_in, center, stages = args
    from scipy.signal import resample_poly
    x = synth.fm_capture(n_out + 64, fs=FS_OUT, seed=seed, channel=k)["iq"].astype(np.complex128)
    for up, down in stages:
        x = resample_poly(x, up, down)
    x = x[:n_in]
    n = np.arange(n_in, dtype=np.float64)
    return (x * np.exp(2j * np.pi * ((center / fs_in * n) % 1.0))).astype(np.complex64)


def _wide_capture(n_st, seed, n_out, n_in, fs_in, centers, stages):
    from concurrent.futures import ProcessPoolExecutor
    workers = min(n_st, 16, max(1, os.cpu_count() or 1))
    wide = None
    with ProcessPoolExecutor(workers) as ex:
        for part in ex.map(_station, [(k, seed, n_out, n_in, fs_in, centers[k], stages) for k in range(n_st)]):
            wide = part.astype(np.complex128) if wide is None else wide + part
    return wide / n_st                                    # as an ADC would see it: the sum scaled into range


def _demodulate(pkg, torch, ch, blocks, n_st, bs):
    """channeliser -> tolerance-mode BatchDemod, block by block: (audio [C, n, 2], RDS bytes per station)"""
    dm = pkg.BatchDemod(n_st, bs, int(FS_OUT), fast_math=True)
    audio, rds = [], [[] for _ in range(n_st)]
    for blk in blocks:
        y = ch.process(blk)
        assert tuple(y.shape) == (n_st, bs, 2)
        dm.process(y.contiguous())
        audio.append(dm.audio())
        byt, cnt = dm.rds_bytes()
        for k in range(n_st):
            rds[k].append(bytes(byt[k, :cnt[k]]))
    dm.close()
    return np.concatenate(audio, axis=1), [b"".join(r) for r in rds]


def _pi_decoded(rds, n_st):
    return [k for k in range(n_st) if (0x1234 + k) in {g[0] for g in decode_groups(np.frombuffer(rds[k], np.uint8))}]


def test_rtl_sdr_u8_capture_end_to_end(pkg):
    """Six FM stations in one 2.4 MSa/s capture quantised as an RTL-SDR delivers it (synth.to_u8: round(127 + 100 x)) -> the channeliser
    reading the u8 capture -> the tolerance-mode demodulator.  Audio and RDS bytes are those of the same chain fed the capture's cf32
    conversion, bit for bit; every station's own PI code decodes."""
    import torch
    fs_in, n_st, bs, nb = 2.4e6, 6, 16384, 10
    n_out = bs * nb
    n_in = n_out * 75 // 8
    centers = np.array([-1.0e6, -0.6e6, -0.2e6, 0.2e6, 0.6e6, 1.0e6])
    wide = _wide_capture(n_st, 900, n_out, n_in, fs_in, centers, [(75, 8)])
    u8 = synth.to_u8(wide)
    assert u8.min() < 80 and u8.max() > 175                  # the capture uses the converter's range
    step = bs * 75 // 8
    got = {}
    for fmt, arr in (("u8", u8), ("cf32", synth.u8_to_cf32(u8))):
        dev = _dev(torch, arr)
        ch = pkg.Channelizer(fs_in, centers, max_input_samples=step)
        got[fmt] = _demodulate(pkg, torch, ch, [dev[b * step:(b + 1) * step] for b in range(nb)], n_st, bs)
        ch.close()
    (a_u8, rds_u8), (a_f, rds_f) = got["u8"], got["cf32"]
    assert np.array_equal(a_u8, a_f)
    assert rds_u8 == rds_f
    pis = _pi_decoded(rds_u8, n_st)
    print(f"RTL-SDR u8 at 2.4 MSa/s, {n_st} stations: PI codes decoded {len(pis)} / {n_st}")
    assert pis == list(range(n_st)), pis


def test_hackrf_s8_whole_band_end_to_end(pkg):
    """16 FM stations across +-9.9 MHz in one 20 MSa/s capture quantised to s8 as a HackRF delivers it (round(100 x)) -> the channeliser
    (k_channelize_band_mfma) reading the s8 capture -> the tolerance-mode demodulator: every station's own PI code decodes."""
    import torch
    fs_in, n_st, bs, nb = 20e6, 16, 16384, 10
    n_out = bs * nb
    n_in = n_out * 625 // 8
    centers = np.linspace(-9.9e6, 9.9e6, n_st)
    # 256 k -> 2.56 M -> 20 M: two short interpolation filters instead of one 625 / 8 filter of 12501 taps
    wide = _wide_capture(n_st, 950, n_out, n_in, fs_in, centers, [(10, 1), (125, 16)])
    s8 = np.empty((n_in, 2), np.int8)
    s8[:, 0] = np.clip(np.rint(100.0 * wide.real), -128, 127)
    s8[:, 1] = np.clip(np.rint(100.0 * wide.imag), -128, 127)
    del wide
    step = bs * 625 // 8
    dev = _dev(torch, s8)
    ch = pkg.Channelizer(fs_in, centers, max_input_samples=step)
    _, rds = _demodulate(pkg, torch, ch, [dev[b * step:(b + 1) * step] for b in range(nb)], n_st, bs)
    ch.close()
    pis = _pi_decoded(rds, n_st)
    print(f"HackRF s8 at 20 MSa/s, {n_st} stations: PI codes decoded {len(pis)} / {n_st}")
    assert pis == list(range(n_st)), pis
