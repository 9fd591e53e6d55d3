"""Batched loudness meter on the GPU (fmd_meter_*, LoudnessMeter): status records, histograms and peaks against the C restatement of the
arithmetic contract (tests/cpp/meter_ref.c, itself checked in test_meter_cpu.py), bit for bit: one call, split calls on alternating
streams, batch and row invariance, the `active` mask, resets, zero / inf / NaN input, a resampler's output at 48 kHz, the known answer of
EBU Tech 3341, the C++ adaptor behind the demodulator, and argument errors."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import meter_ref
import synth
from meter_ref import bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FS = 32000
N1 = 3 * 3200 + 777


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return meter_ref.build(tmp_path_factory.mktemp("meter_ref_gpu"))


@pytest.fixture(scope="module")
def x1():
    """test 1's audio: [3, N1, 2] noise with a 60 dB level step, a different level per station"""
    return meter_ref.stepped_noise(3, N1)


@pytest.fixture(scope="module")
def basic(pkg, ref, x1):
    """test 1's result: (status [3], hist [3, 1000]) after one call, already checked against the restatement"""
    m = pkg.LoudnessMeter(3, FS)
    m.process(_cuda(x1))
    st, hist = m.status(), m.histogram()
    m.close()
    return st, hist


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got_st, got_hist, chans, what=""):
    """device records and histograms == the restatement's stations, bit for bit"""
    for c, ch in enumerate(chans):
        want = ch.status()[0]
        for f in meter_ref.STATUS_DTYPE.names:
            assert np.array_equal(bits(got_st[c][f]), bits(want[f])), (what, c, f, got_st[c][f], want[f])
        assert np.array_equal(got_hist[c], ch.hist()), (what, c, np.flatnonzero(got_hist[c] != ch.hist()))


def _without_peak_call(st):
    st = st.copy()
    st["peak_call"] = 0
    return st


def test_basic_one_call(pkg, ref, x1, basic):
    st, hist = basic
    chans = [ref.run(FS, x1[c]) for c in range(3)]
    _same(st, hist, chans, "one call")
    assert [int(v) for v in st["subblocks"]] == [3, 3, 3] and [int(v) for v in st["frames"]] == [N1] * 3
    assert np.isfinite(st["energy_ring"]).all() and (st["energy_ring"][:, :3] > 0).all() and not hist.any()
    # the same audio twice more, so that gating blocks exist (six per station)
    m = pkg.LoudnessMeter(3, FS)
    for k in range(3):
        m.process(_cuda(x1))
        if k:
            for c in range(3):
                chans[c].process(x1[c])
        _same(m.status(), m.histogram(), chans, f"call {k}")
    st, hist = m.status(), m.histogram()
    assert [int(v) for v in st["subblocks"]] == [9, 9, 9]
    assert (hist.sum(1) > 0).all() and (hist.sum(1) + st["below_gate"] == 6).all()
    want = [ch.integrated() for ch in chans]
    assert np.array_equal(bits(m.integrated(hist)), bits(np.array(want)))
    for c in range(3):
        assert pkg.meter_momentary(st[c]) == chans[c].momentary()
        with pytest.raises(pkg.FmdError) as e:
            pkg.meter_short_term(st[c])
        assert e.value.status == -6
    assert m.status_dev_ptr()


def test_splits_on_alternating_streams_with_a_padded_stride(pkg, ref, x1, basic):
    """calls of 1, 2047 and the rest, on two alternating streams, in_stride > n: everything but peak_call (which is per call by
    definition) equals the one-call result, and the whole record equals the restatement fed the same pieces"""
    import torch
    xp = torch.zeros(3, N1 + 9, 2, device="cuda")
    xp[:, :N1] = _cuda(x1)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    m = pkg.LoudnessMeter(3, FS)
    chans = [ref.channel(FS) for _ in range(3)]
    for k, (a, b) in enumerate(((0, 1), (1, 2048), (2048, N1))):
        m.process(xp[:, a:], n=b - a, stream=streams[k % 2])
        for c in range(3):
            chans[c].process(x1[c, a:b])
    st, hist = m.status(), m.histogram()
    _same(st, hist, chans, "splits")
    assert np.array_equal(bits(_without_peak_call(st)), bits(_without_peak_call(basic[0]))) and np.array_equal(hist, basic[1])


def test_batch_and_row_invariance(pkg, ref, x1, basic):
    """C = 65 (one more than a wavefront of stations), station 64 carrying test 1's station 0"""
    rng = np.random.default_rng(8)
    x = (0.1 * rng.standard_normal((65, N1, 2))).astype(np.float32)
    x[64] = x1[0]
    m = pkg.LoudnessMeter(65, FS)
    m.process(_cuda(x))
    st, hist = m.status(), m.histogram()
    assert np.array_equal(bits(st[64]), bits(basic[0][0])) and np.array_equal(hist[64], basic[1][0])
    _same(st, hist, [ref.run(FS, x[c]) for c in range(65)], "C = 65")


def test_active_mask(pkg, ref, x1):
    import torch
    cuts = (0, 3000, 7000, N1)
    m = pkg.LoudnessMeter(3, FS)
    chans = [ref.channel(FS) for _ in range(3)]
    xd = _cuda(x1)
    for k in range(3):
        a, b = cuts[k], cuts[k + 1]
        active = torch.tensor([1, 0 if k == 1 else 1, 1], dtype=torch.uint8, device="cuda")
        m.process(xd[:, a:], n=b - a, active=active if k else None)
        for c in range(3):
            if not (k == 1 and c == 1):
                chans[c].process(x1[c, a:b])
        _same(m.status(), m.histogram(), chans, f"call {k}")        # (station 1 keeps call 0's peak_call through call 1)
    assert int(m.status()[1]["frames"]) == N1 - 4000
    # a bool mask with nothing on changes nothing
    before = m.status()
    m.process(xd, active=torch.zeros(3, dtype=torch.bool, device="cuda"))
    assert np.array_equal(bits(m.status()), bits(before))


def test_reset_and_reset_peaks_touch_only_what_they_name(pkg, ref, x1):
    m = pkg.LoudnessMeter(3, FS)
    chans = [ref.run(FS, x1[c]) for c in range(3)]
    xd = _cuda(x1)
    m.process(xd)
    m.process(xd)
    for c in range(3):
        chans[c].process(x1[c])
    m.reset(1)
    chans[1].reset()
    st, hist = m.status(), m.histogram()
    _same(st, hist, chans, "after reset(1)")
    assert not bits(st[1]).any() and not hist[1].any() and hist[0].any()
    m.reset_peaks(0)
    chans[0].reset_peaks()
    _same(m.status(), m.histogram(), chans, "after reset_peaks(0)")
    assert not m.status()[0]["peak_hold"].any() and m.status()[2]["peak_hold"].all()
    m.process(xd[:, :5000])
    for c in range(3):
        chans[c].process(x1[c, :5000])
    _same(m.status(), m.histogram(), chans, "after the next call")
    m.reset_peaks()
    m.reset()
    assert not bits(m.status()).any() and not m.histogram().any()


def test_extremes(pkg, ref):
    """silence, one inf sample, one NaN sample.  A NaN's sign and payload are not part of the contract (IEEE 754 leaves them to the
    implementation), so NaN energies are compared as NaNs and everything else bit for bit."""
    fs, nsb = 8000, 800
    n = 6 * nsb + 13
    rng = np.random.default_rng(9)
    x = (0.1 * rng.standard_normal((4, n, 2))).astype(np.float32)
    x[0] = 0.0
    x[1, 2 * nsb + 5, 0] = np.inf
    x[2, nsb + 7, 1] = np.nan
    m = pkg.LoudnessMeter(4, fs)
    m.process(_cuda(x))
    st, hist = m.status(), m.histogram()
    chans = [ref.run(fs, x[c]) for c in range(4)]
    _same(st[[0, 3]], hist[[0, 3]], [chans[0], chans[3]], "finite stations")
    for c in (1, 2):
        want = chans[c].status()[0]
        for f in ("frames", "subblocks", "peak_call", "peak_hold", "below_gate", "nonfinite"):
            assert np.array_equal(bits(st[c][f]), bits(want[f])), (c, f, st[c][f], want[f])
        nan = np.isnan(want["energy_ring"])
        assert np.array_equal(np.isnan(st[c]["energy_ring"]), nan)
        assert np.array_equal(bits(st[c]["energy_ring"][~nan]), bits(want["energy_ring"][~nan]))
        assert np.array_equal(hist[c], chans[c].hist())
    # silence: E = 0, every gating block under the gate, integrated -inf, peak 0
    assert not st[0]["energy_ring"].any() and int(st[0]["below_gate"]) == 3 and not hist[0].any()
    assert m.integrated(hist)[0] == -np.inf and not st[0]["peak_hold"].any() and pkg.meter_momentary(st[0]) == -np.inf
    # inf: the sub-block it falls in and every later one are not finite, and the gating blocks that hold one are counted
    assert np.isfinite(st[1]["energy_ring"][:2]).all() and not np.isfinite(st[1]["energy_ring"][2:6]).any()
    assert int(st[1]["nonfinite"]) == 3 and st[1]["peak_hold"][0] == np.inf and np.isfinite(st[1]["peak_hold"][1])
    # NaN: fmaxf keeps the other operand, so the peak is the largest of the other samples
    want = np.nanmax(np.abs(x[2]), axis=0)
    assert np.array_equal(bits(st[2]["peak_hold"]), bits(want)) and not np.isfinite(st[2]["energy_ring"][1:6]).any()
    assert int(st[2]["nonfinite"]) == 3
    # ... until reset
    for c in (1, 2):
        m.reset(c)
        chans[c].reset()
        chans[c].process(x[3])
    chans[0].process(x[3])
    chans[3].process(x[3])
    m.process(_cuda(np.stack([x[3]] * 4)))
    st, hist = m.status(), m.histogram()
    _same(st, hist, chans, "after reset")
    assert np.isfinite(st["energy_ring"]).all()


def test_48k_resampler_output_in_eight_calls(pkg, ref):
    """the meter behind the resampler at 48 kHz: 3072 frames a call, so a sub-block boundary (every 4800) falls inside most calls"""
    import torch
    C = 5
    rng = np.random.default_rng(10)
    a = (0.2 * rng.standard_normal((C, 8 * 2048, 2)) * np.logspace(0, -4, C)[:, None, None]).astype(np.float32)
    rs = pkg.AudioResampler(C, 48000, method="reference", max_input_frames=2048)
    m = pkg.LoudnessMeter(C, 48000, max_input_frames=3072)
    chans = [ref.channel(48000) for _ in range(C)]
    s = torch.cuda.Stream()
    ad = _cuda(a)
    torch.cuda.synchronize()
    ys = []
    for k in range(8):
        with torch.cuda.stream(s):
            y = rs.process(ad[:, k * 2048:(k + 1) * 2048], stream=s)
            m.process(y, stream=s)
            ys.append(y.clone())
    torch.cuda.synchronize()
    for k in range(8):
        yh = ys[k].cpu().numpy()
        assert yh.shape == (C, 3072, 2)
        for c in range(C):
            chans[c].process(yh[c])
    st, hist = m.status(), m.histogram()
    _same(st, hist, chans, "48 kHz")
    assert [int(v) for v in st["subblocks"]] == [5] * C and (hist.sum(1) + st["below_gate"] == 2).all() and hist.sum() > 0


def test_known_answer_on_the_device(pkg, ref):
    """a stereo 1 kHz sine at -23 dBFS per rail, 5 s at 32 kHz: -23.0 +- 0.1 LU (EBU Tech 3341), and the restatement's values exactly"""
    x = meter_ref.sine(FS, 5.0, 1000.0, -23.0, -23.0)
    ch = ref.run(FS, x)
    m = pkg.LoudnessMeter(1, FS, max_input_frames=x.shape[0])
    m.process(_cuda(x[None]))
    st, hist = m.status(), m.histogram()
    _same(st, hist, [ch], "sine")
    got = (m.integrated(hist)[0], pkg.meter_momentary(st[0]), pkg.meter_short_term(st[0]))
    print("integrated, momentary, short-term:", got)
    for v, want in zip(got, (ch.integrated(), ch.momentary(), ch.short_term())):
        assert abs(v + 23.0) <= 0.1
        assert v == want


def test_cpp_adaptor_behind_the_demodulator(pkg, tmp_path):
    """tests/cpp/meter_main.cpp meters fmd_audio_dev's view of two blocks of one synthetic station; the record it prints is the record
    Python gets from the same audio"""
    exe = tmp_path / "meter_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}",
                    str(ROOT / "tests" / "cpp" / "meter_main.cpp"), f"-L{csrc}", "-lfmdemod", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    bs, nb = 16384, 2
    cap = synth.to_cf32(synth.fm_capture(bs * nb, fs=256000.0, seed=71, channel=1)["iq"])[None]
    np.ascontiguousarray(cap).tofile(tmp_path / "cap.cf32")
    out = subprocess.run([str(exe), str(tmp_path / "cap.cf32"), "1", str(bs), "256000"], check=True, capture_output=True, text=True).stdout.split()
    dm = pkg.BatchDemod(1, bs, 256_000)
    m = pkg.LoudnessMeter(1, 32000)
    for b in range(nb):
        dm.process(np.ascontiguousarray(cap[:, b * bs:(b + 1) * bs]))
        dm.synchronize()
        m.process(dm.audio_tensor())
    st, hist = m.status(), m.histogram()
    dm.close()
    assert int(st[0]["frames"]) == nb * bs // 8 and int(st[0]["subblocks"]) == 1 and st[0]["peak_hold"].all()
    assert bytes.fromhex(out[0]) == st[0].tobytes()
    assert float(out[1]) == m.integrated(hist)[0] and int(out[2]) == int(hist.sum())


def test_argument_errors_change_nothing(pkg, x1):
    import torch
    m = pkg.LoudnessMeter(3, FS, max_input_frames=4096)
    xd = _cuda(x1)
    m.process(xd[:, :4000])
    before_st, before_hist = m.status(), m.histogram()
    bad = [lambda: m.process(xd, n=N1 + 1),                       # n > in_stride
           lambda: m.process(xd, n=4097),                         # n > max_input_frames
           lambda: m.process(xd, n=-1),
           lambda: m.reset(3), lambda: m.reset(-2), lambda: m.reset_peaks(3), lambda: m.reset_peaks(-2)]
    for k, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as e:
            f()
        assert e.value.status == -1, k                            # FMD_ERR_ARG
    # the binding refuses what does not have the meter's shape before the library is called
    for f in (lambda: m.process(xd[:2]), lambda: m.process(xd, active=torch.ones(2, dtype=torch.uint8, device="cuda")),
              lambda: m.process(xd.double()), lambda: m.process(xd[:, :, :1])):
        with pytest.raises(ValueError):
            f()
    # a pointer that is not aligned to a frame
    with pytest.raises(pkg.FmdError) as e:
        m._check(m.L.fmd_meter_process_f32_dev(m.m, xd.data_ptr() + 4, N1, 16, None, None))
    assert e.value.status == -1
    for cfg in ((0, FS, 64), (3, 44101, 64), (3, FS, 0)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.LoudnessMeter(cfg[0], cfg[1], max_input_frames=cfg[2])
        assert e.value.status == -1
    assert np.array_equal(bits(m.status()), bits(before_st)) and np.array_equal(m.histogram(), before_hist)
    # n == 0 is valid: it meters nothing and starts a new call's peak
    m.process(xd, n=0)
    st = m.status()
    assert not st["peak_call"].any() and np.array_equal(bits(_without_peak_call(st)), bits(_without_peak_call(before_st)))
