"""Wideband channeliser (BASELINE configs[4]).  The reference has no channeliser, so PARITY IS UNPINNED;
these tests validate by construction:
  * the prototype filter against its specification (CPU, no GPU),
  * the kernel against a float64 restatement of its definition (mix, then polyphase L/M decimation with the library's taps),
  * streaming continuity (one call == many calls), tone isolation between stations,
  * end to end: FM stations placed in a 10 MSa/s capture come out of channeliser + demodulator with their own RDS PI codes and
    audio matching the directly demodulated station within the north-star tolerance.
"""
import numpy as np
import pytest

import synth
from rds_groups import decode_groups

FS_IN, FS_OUT = 10_000_000.0, 256_000.0
# white noise against the float64 definition, max|y - ref| / max|ref| over the whole output: twice the worst figure measured on an MI355X
# over this file's four cases (2.70e-6, the 640-tap matrix-core case; DESIGN.md §6 "Tap placement"), in place of the 2e-5 the tests had
NOISE_BAR = 5.4e-6


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    return p


def ref_channelize(x, f_hz, taps, L, M, fs_in=FS_IN):
    """float64 restatement: y[o] = sum_t taps[t, p] * (x * exp(-j 2 pi f n / fs))[n0 - t], n0 = o M // L, p = (o M) % L."""
    T = taps.shape[0]
    n = np.arange(x.size, dtype=np.float64)
    xm = x.astype(np.complex128) * np.exp(-2j * np.pi * ((f_hz / fs_in * n) % 1.0))
    n_out = x.size * L // M
    o = np.arange(n_out, dtype=np.int64)
    n0, p = (o * M) // L, (o * M) % L
    idx = n0[:, None] - np.arange(T)[None, :]
    g = np.where(idx >= 0, xm[np.clip(idx, 0, None)], 0.0)
    return (g * taps.astype(np.float64)[np.arange(T)[None, :], p[:, None]]).sum(axis=1)


def test_prototype_filter_meets_its_specification(pkg):
    taps, L, M = pkg.chan_design(FS_IN, FS_OUT, 640)
    assert (L, M) == (16, 625) and taps.shape == (640, 16)
    h = taps.astype(np.float64).reshape(-1)              # [t][p] flattened == prototype order n = t L + p
    fs_up = L * FS_IN
    f = np.concatenate([np.linspace(0, 100e3, 41), np.linspace(156e3, 5e6, 400)])
    H = np.abs(np.exp(-2j * np.pi * np.outer(f / fs_up, np.arange(h.size))) @ h) / L
    assert np.all(np.abs(20 * np.log10(H[:41])) < 0.1)   # pass band +-100 kHz flat to 0.1 dB
    assert np.all(20 * np.log10(H[41:]) < -55.0)         # everything that would alias into it is 55 dB down
    assert abs(h.sum() - L) < 1e-3
    with pytest.raises(Exception):
        pkg.chan_design(10e6, 256e3 + 0.5, 640)          # non-integer rate


pytest_gpu = pytest.mark.gpu


@pytest_gpu
def test_kernel_matches_float64_definition_and_streams(pkg):
    import torch
    rng = np.random.default_rng(3)
    n_in = 625 * 96                                      # -> 1536 outputs per station
    x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
    centers = np.array([-4.3e6, -250e3, 0.0, 137e3, 1.0e6, 4.9e6])
    ch = pkg.Channelizer(FS_IN, centers, max_input_samples=n_in)
    taps = ch.taps()
    xt = torch.from_numpy(np.ascontiguousarray(x).view(np.float32).reshape(-1, 2)).cuda()
    y = ch.process(xt).cpu().numpy()
    y = y[..., 0] + 1j * y[..., 1]
    assert y.shape == (6, 1536)
    assert (ch.form, ch.tile_outputs) == ("k_channelize16_mfma", 128)
    worst = 0.0
    for k, f in enumerate(centers):
        ref = ref_channelize(x, f, taps, ch.interp, ch.decim)
        worst = max(worst, float(np.abs(y[k] - ref).max() / np.abs(ref).max()))
    print(f"k_channelize16_mfma, T = 640: max|y - ref| / max|ref| = {worst:.2e}")
    assert worst < NOISE_BAR, worst
    # streaming: the same capture in three unequal calls gives the same samples (history + mixer phase carry over)
    ch.reset()
    parts = [625 * 20, 625 * 33, 625 * 43]
    outs, pos = [], 0
    for n in parts:
        outs.append(ch.process(xt[pos:pos + n].contiguous()).cpu().numpy())
        pos += n
    y2 = np.concatenate(outs, axis=1)
    y2 = y2[..., 0] + 1j * y2[..., 1]
    assert np.abs(y2 - y).max() <= 5e-6 * np.abs(y).max()    # (the mixer's phasor is re-seeded exactly per tile and advanced by recurrence: up to 4.5e-6 of drift on one sample, far less on a sum over 640)
    with pytest.raises(Exception):
        ch.process(xt[:1000].contiguous())               # 1000 inputs is not a whole number of outputs
    # the shortest legal calls, 625 inputs -> 16 outputs: shorter than the 639-sample history (the history hand-over
    # used to be an overlapping device memcpy here), alternating between two streams, into an output buffer with spare capacity
    # (row stride = capacity, not n_out)
    ch.reset()
    bigs = [torch.full((6, 40, 2), 7.0, device="cuda") for _ in range(2)]   # one per stream: the library orders its own work, not the test's reads
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for i in range(96):
        st = streams[i & 1]
        with torch.cuda.stream(st):
            big = bigs[i & 1]
            # (the stream as its raw pointer and as the torch.cuda.Stream itself, each form on both streams)
            got = ch.process(xt[i * 625:(i + 1) * 625].contiguous(), out=big, stream=st if i & 2 else st.cuda_stream)
            assert tuple(got.shape) == (6, 16, 2)
            outs.append(got.clone())
            assert float(big[:, 16:].min()) == 7.0       # nothing written beyond n_out in any row
    torch.cuda.synchronize()
    y3 = torch.cat(outs, dim=1).cpu().numpy()
    y3 = y3[..., 0] + 1j * y3[..., 1]
    assert np.abs(y3 - y).max() <= 5e-6 * np.abs(y).max()
    ch.close()


@pytest_gpu
@pytest.mark.parametrize("fs_out,tpp,form", [(256e3, 768, "16 branches on the VALU (k_channelize16)"), (200e3, 128, "one output per thread (k_channelize)"),
                                             (256e3, 512, "16 branches on the matrix cores (k_channelize16_mfma)")])
def test_the_other_kernel_forms_match_the_float64_definition(pkg, fs_out, tpp, form):
    """The default configuration (16 / 625, 640 taps per phase) runs k_channelize16_mfma, and so does every tap count up to 644 (512
    here); 704 to 1024 taps per phase in multiples of 64 run 16 branches on the VALU (k_channelize16), other rate pairs one output per
    thread (k_channelize).  Same check as above, incl. a call that ends in a partial tile; each case asserts the form it runs."""
    import torch
    rng = np.random.default_rng(4)
    taps, L, M = pkg.chan_design(FS_IN, fs_out, tpp)
    n_in = M * (200 // L + 3) * (16 // np.gcd(16, L))
    x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
    centers = np.array([-3.1e6, 0.0, 2.2e6])
    ch = pkg.Channelizer(FS_IN, centers, fs_out=fs_out, max_input_samples=n_in, taps_per_phase=tpp)
    assert (ch.interp, ch.decim) == (L, M)
    assert f"({ch.form})" in form and ch.tile_outputs == 128, (form, ch.form)
    xt = torch.from_numpy(np.ascontiguousarray(x).view(np.float32).reshape(-1, 2)).cuda()
    y = ch.process(xt).cpu().numpy()
    y = y[..., 0] + 1j * y[..., 1]
    worst = 0.0
    for k, f in enumerate(centers):
        ref = ref_channelize(x, f, ch.taps(), L, M)
        assert y.shape[1] == ref.size
        worst = max(worst, float(np.abs(y[k] - ref).max() / np.abs(ref).max()))
    print(f"{form}, T = {tpp}: max|y - ref| / max|ref| = {worst:.2e}")
    assert worst < NOISE_BAR, (form, worst)
    # streamed (only the matrix-core form had its history hand-over checked across calls): the same capture in several
    # calls — uneven ones, and then the SHORTEST legal calls (one M-sample step of the rate pair, shorter than the T - 1 samples of
    # history, so a call's window lies in the history buffer and the block at once) — must give the one-shot result
    unit = M * (16 // int(np.gcd(16, L)))                # samples per whole number of outputs (and of 16-output groups where L = 16)
    for cuts in ([0, 3 * unit, 4 * unit, n_in], list(range(0, n_in + 1, unit))):
        ch.reset()
        outs = [ch.process(xt[a:b].contiguous()).clone() for a, b in zip(cuts[:-1], cuts[1:])]
        ys = torch.cat(outs, dim=1).cpu().numpy()
        ys = ys[..., 0] + 1j * ys[..., 1]
        assert ys.shape == y.shape
        assert np.abs(ys - y).max() <= 5e-6 * np.abs(y).max(), (form, len(cuts))
    ch.close()


@pytest_gpu
def test_tone_lands_only_in_its_station(pkg):
    import torch
    n_in = 625 * 128
    centers = (np.arange(40) - 19.5) * 250e3             # BASELINE configs[4]: 40 stations across 10 MSa/s
    ch = pkg.Channelizer(FS_IN, centers, max_input_samples=n_in)
    k0 = 27
    n = np.arange(n_in)
    x = np.exp(2j * np.pi * (((centers[k0] + 30e3) / FS_IN * n) % 1.0)).astype(np.complex64)
    y = ch.process(torch.from_numpy(x.view(np.float32).reshape(-1, 2)).cuda()).cpu().numpy()
    p = (y[..., 0] ** 2 + y[..., 1] ** 2)[:, 256:].mean(axis=1)   # skip the filter's start-up
    assert abs(p[k0] - 1.0) < 1e-3
    others = np.delete(p, k0)
    assert others.max() < 1e-5                           # > 50 dB down everywhere else
    ch.close()


@pytest_gpu
def test_wideband_capture_through_channeliser_and_demodulator(pkg):
    """Four FM stations (own audio tones, own RDS PI) in one 10 MSa/s capture -> channeliser -> batched demodulator."""
    import torch
    from scipy.signal import resample_poly, upfirdn
    bs, nb = 16384, 10
    n_out = bs * nb
    centers = np.array([-3.1e6, -0.4e6, 1.3e6, 4.4e6])
    stations = [synth.fm_capture(n_out, fs=FS_OUT, seed=40 + k, channel=k) for k in range(4)]
    n_in = n_out * 625 // 16
    n = np.arange(n_in, dtype=np.float64)
    wide = np.zeros(n_in, np.complex128)
    for k, st in enumerate(stations):
        up = resample_poly(st["iq"].astype(np.complex128), 625, 16)[:n_in]
        wide += up * np.exp(2j * np.pi * ((centers[k] / FS_IN * n) % 1.0))
    wide = (wide / 4.0).astype(np.complex64)             # as an ADC would see it: the sum scaled into range
    ch = pkg.Channelizer(FS_IN, centers, max_input_samples=bs * 625 // 16)
    hflat = ch.taps().astype(np.float64).reshape(-1)
    ref = []
    for k in range(4):
        xm = wide.astype(np.complex128) * np.exp(-2j * np.pi * ((centers[k] / FS_IN * n) % 1.0))
        ref.append(upfirdn(hflat, xm, ch.interp, ch.decim)[:n_out])
    dm = pkg.BatchDemod(4, bs, int(FS_OUT))
    direct = pkg.BatchDemod(4, bs, int(FS_OUT))
    wt = torch.from_numpy(wide.view(np.float32).reshape(-1, 2)).cuda()
    audio, audio_direct, rds_bytes = [], [], [[] for _ in range(4)]
    step = bs * 625 // 16
    for b in range(nb):
        y = ch.process(wt[b * step:(b + 1) * step].contiguous())
        assert tuple(y.shape) == (4, bs, 2)
        dm.process(y.contiguous())
        audio.append(dm.audio())
        byt, cnt = dm.rds_bytes()
        for k in range(4):
            rds_bytes[k].append(bytes(byt[k, :cnt[k]]))
        blk = np.stack([ref[k][b * bs:(b + 1) * bs] for k in range(4)])
        direct.process(np.ascontiguousarray(np.stack([blk.real, blk.imag], axis=-1).astype(np.float32)))
        audio_direct.append(direct.audio())
    a, ad = np.concatenate(audio, axis=1), np.concatenate(audio_direct, axis=1)
    for k in range(4):
        # `direct` was fed the float64 restatement of the channeliser (scipy upfirdn with the library's taps), so the two
        # audio streams may differ only by the kernel's fp32 rounding, amplified by the FM discriminator
        e = np.sqrt(np.mean((a[k, 4096:] - ad[k, 4096:]) ** 2))
        assert e < 1e-3, (k, e)
        # and the station really is the one that was put there: its own RDS PI code and its own audio tones
        groups = decode_groups(np.frombuffer(b"".join(rds_bytes[k]), np.uint8))
        pis = {g[0] for g in groups}
        assert 0x1234 + k in pis, (k, sorted(hex(p) for p in pis))
        spec = np.abs(np.fft.rfft(a[k, -16384:, 0] * np.hanning(16384)))
        f = np.fft.rfftfreq(16384, 1 / 32000.0)
        assert 900 < f[np.argmax(spec[20:]) + 20] < 1100       # left channel carries the 1 kHz tone
    ch.close(); dm.close(); direct.close()


def _wideband_station(args):
    """(worker process) one station of the wideband capture: its 256 kSa/s FM signal resampled to 10 MSa/s and shifted to its centre"""
    k, n_out, n_in, center = args
    from scipy.signal import resample_poly
    st = synth.fm_capture(n_out, fs=FS_OUT, seed=400 + k, channel=k)
    up = resample_poly(st["iq"].astype(np.complex128), 625, 16)[:n_in]
    n = np.arange(n_in, dtype=np.float64)
    return (up * np.exp(2j * np.pi * ((center / FS_IN * n) % 1.0))).astype(np.complex64)


_WIDE = None


def _reference_channel(args):
    """(worker process) the float64 restatement of the channeliser for one station: mix down, polyphase resample 16 / 625 with the library's taps"""
    k, center, hflat, interp, decim, n_out = args
    from scipy.signal import upfirdn
    wide = _WIDE                      # (inherited through fork: 51 MB that need not be pickled 40 times)
    n = np.arange(wide.size, dtype=np.float64)
    xm = wide.astype(np.complex128) * np.exp(-2j * np.pi * ((center / FS_IN * n) % 1.0))
    y = upfirdn(hflat, xm, interp, decim)[:n_out]
    return np.stack([y.real, y.imag], axis=-1).astype(np.float32)


@pytest_gpu
def test_configs4_end_to_end_40_stations_in_the_tolerance_mode(pkg):
    """BASELINE configs[4] as bench.py --wideband runs it: ONE 10 MSa/s capture holding 40 FM stations on the 250 kHz
    raster -> on-GPU polyphase channeliser (k_channelize16_mfma) -> the batched demodulator in the tolerance mode.  Every station's audio
    against the same demodulator fed the float64 restatement of the channeliser (scipy upfirdn with the library's taps): <= 1e-4 RMS
    behind the start-up; every station's own RDS PI code decoded.  The reference has no channeliser (parity unpinned: SURVEY f3);
    its capture format is the anchor (src/rtl_sdr.cpp:42-46)."""
    import os
    from concurrent.futures import ProcessPoolExecutor

    import torch
    n_st, bs, nb = 40, 16384, 10
    n_out = bs * nb
    n_in = n_out * 625 // 16
    centers = (np.arange(n_st) - 19.5) * 250e3
    workers = min(n_st, max(1, (os.cpu_count() or 8) // 2))
    with ProcessPoolExecutor(workers) as ex:
        parts = list(ex.map(_wideband_station, [(k, n_out, n_in, centers[k]) for k in range(n_st)]))
    wide = (np.sum(parts, axis=0) / n_st).astype(np.complex64)       # as an ADC would see it: the sum scaled into range
    del parts
    ch = pkg.Channelizer(FS_IN, centers, max_input_samples=bs * 625 // 16)
    hflat = ch.taps().astype(np.float64).reshape(-1)
    global _WIDE
    _WIDE = wide
    with ProcessPoolExecutor(workers) as ex:
        ref = list(ex.map(_reference_channel, [(k, centers[k], hflat, ch.interp, ch.decim, n_out) for k in range(n_st)]))
    _WIDE = None
    ref = np.stack(ref)                                              # [40, n_out, 2]
    dm = pkg.BatchDemod(n_st, bs, int(FS_OUT), fast_math=True)
    direct = pkg.BatchDemod(n_st, bs, int(FS_OUT), fast_math=True)
    wt = torch.from_numpy(wide.view(np.float32).reshape(-1, 2)).cuda()
    audio, audio_direct, rds_bytes = [], [], [[] for _ in range(n_st)]
    step = bs * 625 // 16
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
    pis_ok = 0
    for k in range(n_st):
        groups = decode_groups(np.frombuffer(b"".join(rds_bytes[k]), np.uint8))
        pis_ok += int((0x1234 + k) in {g[0] for g in groups})
    print(f"configs[4] end to end, 40 stations, tolerance mode: audio vs float64-channelised worst {max(errs):.2e} median {np.median(errs):.2e}; PI codes decoded {pis_ok} / {n_st}")
    try:
        import test_gpu_realistic as R
        R._record(None, "configs4_40_stations_tolerance_mode", {"audio_rms_vs_float64_channelised_worst": max(errs), "audio_rms_median": float(np.median(errs)),
                                                                  "pi_codes_decoded": pis_ok, "stations": n_st, "blocks": nb})
    except Exception as e:      # noqa: BLE001
        print("not recorded:", e)
    assert max(errs) <= 1e-4, errs
    assert pis_ok == n_st
    ch.close(); dm.close(); direct.close()
