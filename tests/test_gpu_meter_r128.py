"""True peak and loudness range of the batched loudness meter on the GPU (fmd_meter_create_ex, k_meter_tp, k_meter<true>) against the C
restatement (tests/cpp/meter_r128_ref.c, itself checked in test_meter_r128_cpu.py), bit for bit: one call and split calls on alternating
streams, the tile's edges and rows that are only 8-byte aligned, batch and row invariance, the `active` mask, resets, NaN / inf /
denormal samples, the three oversampling factors, the known answers, a resampler's output, the C++ adaptor, and that nothing a meter
without the features reports has moved."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import meter_r128_ref as R
import meter_ref
from meter_ref import bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FS = 32000
TILE = 1024                      # frames per tile of k_meter_tp; one workgroup per station, so there is no station tiling
TP, RG = R.TRUE_PEAK, R.RANGE


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("meter_r128_ref_gpu"))


@pytest.fixture(scope="module")
def x777():
    return meter_ref.stepped_noise(3, 777)


@pytest.fixture(scope="module")
def xrange_():
    """6.5 s at 8 kHz, the lowest rate the meter takes: [3, 52000, 2], 65 sub-blocks, 36 short-term values"""
    return meter_ref.stepped_noise(3, 52000, seed=6)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(m, chans, what="", nan_ok=()):
    """the device's status, histogram, r128 records and range histogram == the restatement's stations, bit for bit; stations in `nan_ok`
    hold NaN energies, whose sign and payload are not part of the contract"""
    st, hist, r128 = m.status(), m.histogram(), m.r128_status()
    rh = m.range_histogram() if m.features & RG else None
    for c, ch in enumerate(chans):
        want = ch.status()[0]
        for f in meter_ref.STATUS_DTYPE.names:
            if c in nan_ok and f == "energy_ring":
                nan = np.isnan(want[f])
                assert np.array_equal(np.isnan(st[c][f]), nan) and np.array_equal(bits(st[c][f][~nan]), bits(want[f][~nan])), (what, c, f)
            else:
                assert np.array_equal(bits(st[c][f]), bits(want[f])), (what, c, f, st[c][f], want[f])
        assert np.array_equal(hist[c], ch.hist()), (what, c)
        w = ch.r128()[0]
        for f in R.R128_DTYPE.names:
            assert np.array_equal(bits(r128[c][f]), bits(w[f])), (what, c, f, r128[c][f], w[f])
        if rh is not None:
            assert np.array_equal(rh[c], ch.range_hist()), (what, c, np.flatnonzero(rh[c] != ch.range_hist()))
        if m.features & TP:
            assert np.all(r128[c]["tp_hold"] >= st[c]["peak_hold"]) and np.all(r128[c]["tp_call"] >= st[c]["peak_call"]), (what, c)
    return st, hist, r128, rh


def _without_call(r):
    r = r.copy()
    r["tp_call"] = 0
    return r


# ---- true peak --------------------------------------------------------------------------------------------------------------------

def test_tp_one_call_splits_on_alternating_streams_and_an_empty_call(pkg, ref, x777):
    import torch
    m = pkg.LoudnessMeter(3, FS, features=TP)
    m.process(_cuda(x777))
    chans = [ref.run(FS, x777[c], TP) for c in range(3)]
    _, _, one, _ = _same(m, chans, "one call")
    assert one["tp_hold"].all() and np.any(one["tp_hold"] > m.status()["peak_hold"])
    assert np.allclose(m.true_peak_dbtp(), 20.0 * np.log10(one["tp_hold"].astype(np.float64)), rtol=0, atol=1e-12)
    assert m.r128_status_dev_ptr()
    # n == 0 is valid: tp_call restarts, nothing else moves (the history neither: the next frames continue the stream)
    m.process(_cuda(x777), n=0)
    got = m.r128_status()
    assert not got["tp_call"].any() and np.array_equal(bits(_without_call(got)), bits(_without_call(one)))
    # 1 + 10 + 11 + 12 + 743: pieces below, at and above the 11 frames of history, on two alternating streams, in_stride > n
    xp = torch.zeros(3, 777 + 5, 2, device="cuda")
    xp[:, :777] = _cuda(x777)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    m2 = pkg.LoudnessMeter(3, FS, features=TP)
    chans2 = [ref.channel(FS, TP) for _ in range(3)]
    a = 0
    for k, n in enumerate((1, 10, 11, 12, 743)):
        m2.process(xp[:, a:], n=n, stream=streams[k % 2])
        for c in range(3):
            chans2[c].process(x777[c, a:a + n])
        a += n
    _, _, split, _ = _same(m2, chans2, "splits")
    assert np.array_equal(bits(split["tp_hold"]), bits(one["tp_hold"]))
    # the history the first meter carries through its empty call is the one the second built from pieces: both continue alike
    for mm, cc in ((m, chans), (m2, chans2)):
        mm.reset_peaks()
        mm.process(_cuda(x777[:, :40]))
        for c in range(3):
            cc[c].reset_peaks()
            cc[c].process(x777[c, :40])
    _same(m, chans, "continued")
    _same(m2, chans2, "continued after splits")
    assert np.array_equal(bits(m.r128_status()), bits(m2.r128_status()))


@pytest.mark.parametrize("n", [TILE + 1, 2 * TILE - 1, 2 * TILE])
def test_tp_tile_edges_and_rows_aligned_to_8_bytes_only(pkg, ref, n):
    """an odd n makes every second station's row start 8 bytes off a 16-byte boundary (the kernel's narrow loads); the peak sits in the
    last frame of one station and just behind a tile's edge in another"""
    rng = np.random.default_rng(30 + n)
    x = (0.1 * rng.standard_normal((4, n, 2))).astype(np.float32)
    x[1, n - 1, 0] = 0.9
    x[2, TILE, 1] = -0.8
    x[3, TILE - 1, 0] = 0.7
    m = pkg.LoudnessMeter(4, FS, features=TP)
    m.process(_cuda(x))
    chans = [ref.run(FS, x[c], TP) for c in range(4)]
    _same(m, chans, f"n = {n}")
    # and once more, so that the history carried over a tile-sized call is used
    m.process(_cuda(x))
    for c in range(4):
        chans[c].process(x[c])
    _same(m, chans, f"n = {n}, second call")


def test_tp_batch_and_row_invariance(pkg, ref):
    rng = np.random.default_rng(31)
    x = (0.1 * rng.standard_normal((5, 777, 2))).astype(np.float32)
    m = pkg.LoudnessMeter(5, FS, features=TP | RG)
    m.process(_cuda(x))
    batch = m.r128_status()
    _same(m, [ref.run(FS, x[c]) for c in range(5)], "batch of 5")
    for k in (0, 3, 4):
        m1 = pkg.LoudnessMeter(1, FS, features=TP | RG)
        m1.process(_cuda(x[k:k + 1]))
        assert np.array_equal(bits(m1.r128_status()[0]), bits(batch[k])), k
        assert np.array_equal(bits(m1.status()[0]), bits(m.status()[k])), k


def test_tp_active_mask_resets_and_history(pkg, ref, x777):
    import torch
    m = pkg.LoudnessMeter(3, FS, features=TP | RG)
    chans = [ref.channel(FS) for _ in range(3)]
    xd = _cuda(x777)
    cuts = (0, 300, 305, 777)
    for k in range(3):
        a, b = cuts[k], cuts[k + 1]
        active = torch.tensor([1, 0 if k == 1 else 1, 1], dtype=torch.uint8, device="cuda")
        m.process(xd[:, a:], n=b - a, active=active if k else None)
        for c in range(3):
            if not (k == 1 and c == 1):
                chans[c].process(x777[c, a:b])
        _same(m, chans, f"call {k}")          # station 1 keeps call 0's tp_call and history through call 1, and call 2 continues from them
    before = m.r128_status()
    m.process(xd, active=torch.zeros(3, dtype=torch.bool, device="cuda"))
    assert np.array_equal(bits(m.r128_status()), bits(before))
    # reset_peaks clears the four floats and keeps the history: a quiet continuation reads the tail of what came before
    m.reset_peaks(0)
    chans[0].reset_peaks()
    _same(m, chans, "after reset_peaks(0)")
    assert not m.r128_status()[0]["tp_hold"].any() and m.r128_status()[2]["tp_hold"].all()
    quiet = np.zeros((3, 5, 2), np.float32)
    m.process(_cuda(quiet))
    for c in range(3):
        chans[c].process(quiet[c])
    _, _, r, _ = _same(m, chans, "quiet continuation")
    assert r[0]["tp_call"].all()                                                 # zeros in, the history's ringing out
    # reset clears the history too: the same quiet frames now read 0
    m.reset(0)
    chans[0].reset()
    m.process(_cuda(quiet))
    for c in range(3):
        chans[c].process(quiet[c])
    _, _, r, _ = _same(m, chans, "after reset(0)")
    assert not bits(r[0]).any() and r[2]["tp_hold"].all()
    m.reset()
    assert not bits(m.r128_status()).any() and not m.range_histogram().any()


def test_tp_nan_inf_and_denormal_samples(pkg, ref):
    rng = np.random.default_rng(32)
    n = 1500
    x = (0.1 * rng.standard_normal((4, n, 2))).astype(np.float32)
    x[0, 700, 0] = np.nan
    x[1, 1030, 1] = np.inf
    x[2] = (x[2].astype(np.float64) * 1e-38).astype(np.float32)                  # denormals, and products that are
    x[3] = 0.0
    x[3, 5, 0] = np.float32(1e-45)                                               # the smallest denormal alone
    assert np.any((np.abs(x[2]) < 1.1754944e-38) & (x[2] != 0))
    m = pkg.LoudnessMeter(4, FS, features=TP)
    m.process(_cuda(x))
    chans = [ref.run(FS, x[c], TP) for c in range(4)]
    _, _, r, _ = _same(m, chans, "extremes", nan_ok=(0, 1))
    assert np.isfinite(r[0]["tp_hold"]).all() and r[0]["tp_hold"].all()          # the NaN is dropped, with every output it touches
    assert r[1]["tp_hold"][1] == np.inf and np.isfinite(r[1]["tp_hold"][0])
    assert 0 < r[2]["tp_hold"][0] < 1e-37 and r[3]["tp_hold"][0] == np.float32(1e-45) and r[3]["tp_hold"][1] == 0


@pytest.mark.parametrize("fs", [96000, 192000])
def test_tp_two_times_and_no_oversampling(pkg, ref, fs, x777):
    assert pkg.meter_tp_design(fs).L == (2 if fs == 96000 else 1)
    m = pkg.LoudnessMeter(3, fs, features=TP)
    chans = [ref.channel(fs, TP) for _ in range(3)]
    for a, b in ((0, 9), (9, 777)):
        m.process(_cuda(x777[:, a:b]))
        for c in range(3):
            chans[c].process(x777[c, a:b])
    st, _, r, _ = _same(m, chans, f"fs {fs}")
    if fs == 192000:
        assert np.array_equal(bits(r["tp_hold"]), bits(st["peak_hold"])) and np.array_equal(bits(r["tp_call"]), bits(st["peak_call"]))
    else:
        assert np.any(r["tp_hold"] > st["peak_hold"])


@pytest.mark.parametrize("fs", [32000, 48000])
def test_tp_known_answers_on_the_device(pkg, ref, fs):
    """the five sines of test_meter_r128_cpu.py as five stations: the restatement's values exactly, inside EBU Tech 3341's +0.2 / -0.4 dB"""
    x = np.stack([R.tp_sine(4000, amp, div, ph) for amp, div, ph, _ in R.TP_SINES])
    m = pkg.LoudnessMeter(5, fs, features=TP)
    m.process(_cuda(x))
    _same(m, [ref.run(fs, x[c], TP) for c in range(5)], "sines")
    got = m.true_peak_dbtp()
    print(fs, "dBTP:", got[:, 0])
    for c, (_, _, _, want) in enumerate(R.TP_SINES):
        assert np.all(got[c] - want <= R.TP_TOL[1]) and np.all(got[c] - want >= R.TP_TOL[0]), (c, got[c], want)
    sample = pkg.meter_dbtp(m.status()["peak_hold"])
    assert np.all(np.abs(sample[1] - (R.TP_SINES[1][3] - 3.0103)) < 0.01)


def test_tp_behind_the_resampler_at_48k(pkg, ref):
    import torch
    C = 2
    rng = np.random.default_rng(33)
    a = (0.2 * rng.standard_normal((C, 2 * 2048, 2))).astype(np.float32)
    rs = pkg.AudioResampler(C, 48000, method="reference", max_input_frames=2048)
    m = pkg.LoudnessMeter(C, 48000, max_input_frames=3072, features=TP | RG)
    chans = [ref.channel(48000) for _ in range(C)]
    s = torch.cuda.Stream()
    ad = _cuda(a)
    torch.cuda.synchronize()
    ys = []
    for k in range(2):
        with torch.cuda.stream(s):
            y = rs.process(ad[:, k * 2048:(k + 1) * 2048], stream=s)
            m.process(y, stream=s)
            ys.append(y.clone())
    torch.cuda.synchronize()
    for k in range(2):
        yh = ys[k].cpu().numpy()
        for c in range(C):
            chans[c].process(yh[c])
    _same(m, chans, "48 kHz")


# ---- range ------------------------------------------------------------------------------------------------------------------------

def _check_range(pkg, m, chans, what):
    st, _, r, rh = _same(m, chans, what)
    G = st["subblocks"].astype(np.int64)
    assert np.array_equal(rh.sum(1) + r["st_below"] + r["st_nonfinite"], np.maximum(0, G - 29)), what
    lra, low, high = m.loudness_range()
    for c, ch in enumerate(chans):
        want = ch.loudness_range()
        if want is None:
            assert np.isnan(lra[c]) and np.isnan(low[c]) and np.isnan(high[c]), (what, c)
        else:
            assert (lra[c], low[c], high[c]) == want, (what, c)
    return st, r, rh, lra


def test_range_one_call_that_completes_65_subblocks(pkg, ref, xrange_):
    m = pkg.LoudnessMeter(3, 8000, features=RG)
    m.process(_cuda(xrange_))
    chans = [ref.run(8000, xrange_[c], RG) for c in range(3)]
    st, r, rh, lra = _check_range(pkg, m, chans, "one call")
    assert [int(v) for v in st["subblocks"]] == [65] * 3 and rh.sum() > 0 and np.isfinite(lra).any()
    assert not r["tp_call"].any() and not r["tp_hold"].any()                     # the feature that is off stays 0
    with pytest.raises(pkg.FmdError) as e:
        m.true_peak_dbtp()
    assert e.value.status == -6


def test_range_calls_cut_around_subblock_ends(pkg, ref, xrange_):
    """799, 800, 801 frames repeated (a sub-block is 800): ends fall in the last frame of a call, in the first, and between"""
    m = pkg.LoudnessMeter(3, 8000, features=TP | RG)
    chans = [ref.channel(8000) for _ in range(3)]
    xd = _cuda(xrange_)
    a, k = 0, 0
    while a < xrange_.shape[1]:
        n = min((799, 800, 801)[k % 3], xrange_.shape[1] - a)
        m.process(xd[:, a:], n=n)
        for c in range(3):
            chans[c].process(xrange_[c, a:a + n])
        a, k = a + n, k + 1
    _, _, rh, _ = _check_range(pkg, m, chans, "799 / 800 / 801")
    one = [ref.run(8000, xrange_[c], RG) for c in range(3)]
    assert all(np.array_equal(rh[c], one[c].range_hist()) for c in range(3))


def test_range_silence_and_inf(pkg, ref):
    rng = np.random.default_rng(34)
    n = 33 * 800 + 7
    x = (0.1 * rng.standard_normal((3, n, 2))).astype(np.float32)
    x[0] = 0.0
    x[1, 20 * 800 + 3, 0] = np.inf
    m = pkg.LoudnessMeter(3, 8000, features=RG)
    m.process(_cuda(x))
    chans = [ref.run(8000, x[c], RG) for c in range(3)]
    st, hist, r, rh = _same(m, chans, "extremes", nan_ok=(1,))
    assert int(r[0]["st_below"]) == 4 and not rh[0].any() and int(r[0]["st_nonfinite"]) == 0
    assert int(r[1]["st_nonfinite"]) == 4 and not rh[1].any()
    assert int(rh[2].sum()) == 4 and int(r[2]["st_below"]) == 0
    lra = m.loudness_range()[0]
    assert np.isnan(lra[0]) and np.isnan(lra[1]) and lra[2] >= 0.0


# ---- nothing else moved -----------------------------------------------------------------------------------------------------------

def test_features_leave_the_meter_itself_alone(pkg, xrange_):
    xd = _cuda(xrange_)
    got = {}
    for feat in (0, TP, RG, TP | RG):
        m = pkg.LoudnessMeter(3, 8000, features=feat)
        for a, b in ((0, 30001), (30001, 52000)):
            m.process(xd[:, a:], n=b - a)
        got[feat] = (m.status(), m.histogram())
        if feat == 0:
            for f in (m.r128_status, m.range_histogram, m.r128_status_dev_ptr, m.true_peak_dbtp, m.loudness_range):
                with pytest.raises(pkg.FmdError) as e:
                    f()
                assert e.value.status == -6, f                                   # FMD_ERR_STATE
        if feat == TP:
            with pytest.raises(pkg.FmdError) as e:
                m.range_histogram()
            assert e.value.status == -6
            assert m.r128_status()["tp_hold"].all()
    assert got[0][1].sum() > 0
    for feat in (TP, RG, TP | RG):
        assert np.array_equal(bits(got[feat][0]), bits(got[0][0])) and np.array_equal(got[feat][1], got[0][1]), feat


def test_feature_bits(pkg):
    import ctypes
    for bad in (4, 8, 7, 1 << 31):
        with pytest.raises(pkg.FmdError) as e:
            pkg.LoudnessMeter(3, FS, features=bad)
        assert e.value.status == -1, bad                                         # FMD_ERR_ARG
    for feat in (0, 1, 2, 3):
        m = pkg.LoudnessMeter(2, FS, features=feat)
        v = ctypes.c_uint(99)
        assert m.L.fmd_meter_features(m.m, ctypes.byref(v)) == 0 and v.value == feat
        m.close()


def test_cpp_adaptor_with_both_features(pkg, ref, tmp_path, xrange_):
    """tests/cpp/meter_r128_adaptor_main.cpp meters a file of audio in calls of 4801 frames; the records it prints are the restatement's"""
    exe = tmp_path / "meter_r128_adaptor_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'fm-radio_amd' / 'host'}", "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "meter_r128_adaptor_main.cpp"),
                    f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)],
                   check=True)
    xrange_.tofile(tmp_path / "audio.f32")
    out = subprocess.run([str(exe), str(tmp_path / "audio.f32"), "3", "8000", "4801"], check=True, capture_output=True, text=True).stdout
    lines = out.strip().split("\n")
    assert len(lines) == 3
    for c, line in enumerate(lines):
        w = line.split()
        ch = ref.channel(8000)
        for a in range(0, 52000, 4801):
            ch.process(xrange_[c, a:a + 4801])
        assert bytes.fromhex(w[0]) == ch.status()[0].tobytes() and bytes.fromhex(w[1]) == ch.r128()[0].tobytes(), c
        assert int(w[2]) == int(ch.range_hist().sum())
        want = ch.loudness_range()
        if want is None:
            assert all(v == "nan" for v in w[3:6])
        else:
            assert tuple(float(v) for v in w[3:6]) == want
        assert float(w[6]) == pkg.meter_dbtp(ch.r128()[0]["tp_hold"][0])
