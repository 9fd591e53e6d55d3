"""True peak and loudness range of the batched loudness meter, the parts that need no GPU: the ABI is declared and exported; the
interpolator's taps from the library, the C restatement (tests/cpp/meter_r128_ref.c) and an independent model, bit for bit; the known
answers of EBU Tech 3341 (true peak) and Tech 3342 (range) through the restatement; fmd_meter_range's edge cases; and the host-only code
in a stand-alone program under the address and undefined-behaviour sanitizers."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import meter_r128_ref as R
from meter_ref import bits

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["fmd_meter_create_ex", "fmd_meter_features", "fmd_meter_tp_design", "fmd_meter_dbtp", "fmd_meter_get_r128_status",
           "fmd_meter_r128_status_dev", "fmd_meter_get_range_histogram", "fmd_meter_range"]
RATES = {8000: 4, 32000: 4, 44100: 4, 48000: 4, 96000: 2, 192000: 1}


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("meter_r128_ref"))


def test_symbols_are_declared_and_exported(pkg):
    declared = pkg.declared_symbols(debug=False)
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/fmdemod.h"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.fmd_api_version() == 3
    for name in ("METER_TRUE_PEAK", "METER_RANGE", "METER_R128_DTYPE", "meter_tp_design", "meter_range", "meter_dbtp"):
        assert hasattr(pkg, name), name
    for name in ("r128_status", "range_histogram", "loudness_range", "true_peak_dbtp"):
        assert hasattr(pkg.LoudnessMeter, name), name
    assert (pkg.METER_TRUE_PEAK, pkg.METER_RANGE) == (1, 2)
    assert pkg.METER_R128_DTYPE == R.R128_DTYPE and pkg.METER_R128_DTYPE.itemsize == 24
    assert [pkg.METER_R128_DTYPE.fields[k][1] for k in ("tp_call", "tp_hold", "st_below", "st_nonfinite")] == [0, 8, 16, 20]


def test_taps_of_library_restatement_and_model_are_the_same_bits(pkg, ref):
    for fs, L in RATES.items():
        d, r = pkg.meter_tp_design(fs), ref.tp_design(fs)
        mL, mt = R.model_tp_design(fs)
        assert d.L == r.L == mL == L and d.taps_per_phase == r.taps_per_phase == 12, fs
        t = R.taps_array(d)
        assert np.array_equal(bits(t), bits(R.taps_array(r))), fs
        assert np.array_equal(bits(t), bits(mt)), fs
        assert not t[L - 1:].any()                                             # unused rows are 0
        for p in range(1, L):
            # phase p is phase L - p read backwards.  The prototype is even about c, so the two phases hold the same twelve doubles in
            # opposite order; only their sums, added in opposite order, may differ, by a few ulp of a double: far below half an ulp of a
            # float except at a rounding tie, so one float ulp is allowed.
            a, b = t[p - 1], t[L - p - 1][::-1]
            assert np.all(np.abs(a - b) <= np.spacing(np.abs(a))), (fs, p)
            assert abs(float(np.sum(t[p - 1].astype(np.float64))) - 1.0) <= 1e-6, (fs, p)
    for fs in (0, 44101, 7990, 192010):
        with pytest.raises(pkg.FmdError) as e:
            pkg.meter_tp_design(fs)
        assert e.value.status == -1, fs
    for v in (0.0, 1.0, 0.5, 1.41, 1e-40, np.inf):
        assert np.array_equal(bits(np.float64(pkg.meter_dbtp(v))), bits(np.float64(ref.lib.meter_r128_dbtp(v)))), v
    assert pkg.meter_dbtp(0.0) == -np.inf and pkg.meter_dbtp(1.0) == 0.0


@pytest.mark.parametrize("fs", [32000, 48000])
def test_known_answer_true_peak_of_sines(ref, fs):
    """a sinusoid's true peak is its amplitude whatever the sampling phase: EBU Tech 3341 allows +0.2 / -0.4 dB"""
    for amp, div, phase, want in R.TP_SINES:
        x = R.tp_sine(4000, amp, div, phase)
        ch = ref.run(fs, x, R.TRUE_PEAK)
        tp = ch.r128()[0]["tp_hold"]
        got = 20.0 * np.log10(tp.astype(np.float64))
        sample = 20.0 * np.log10(ch.status()[0]["peak_hold"].astype(np.float64))
        print(fs, amp, div, phase, "dBTP", got, "sample peak dBFS", sample)
        assert abs(want - 20.0 * np.log10(amp)) < 1e-3
        assert np.all(got - want <= R.TP_TOL[1]) and np.all(got - want >= R.TP_TOL[0]), (amp, div, phase, got)
        assert np.array_equal(bits(ch.r128()[0]["tp_call"]), bits(tp)) and np.all(tp >= ch.status()[0]["peak_hold"])
        if (div, phase) == (4, 45.0):
            assert np.all(np.abs(sample - (want - 3.0103)) < 0.01)             # the sample peak under-reads by 3 dB here
        if amp == 1.41:
            assert np.all(got - 3.0 <= R.TP_TOL[1]) and np.all(got - 3.0 >= R.TP_TOL[0])


def test_true_peak_near_nyquist_is_measured_not_promised(ref):
    """sines at 0.8 and 0.9 of Nyquist over 32 sampling phases: the reading never falls under the sample peak and never over the
    amplitude by more than Tech 3341's +0.2 dB; how far under the amplitude the worst phase reads is printed (DESIGN.md 6f quotes it)"""
    for frac in (0.8, 0.9):
        worst_tp, worst_sample = 0.0, 0.0
        for k in range(32):
            i = np.arange(4000, dtype=np.float64)
            s = 0.5 * np.sin(np.pi * frac * i + 2.0 * np.pi * k / 32.0)
            s[:96] *= 0.5 - 0.5 * np.cos(np.pi * np.arange(96) / 96)
            ch = ref.run(32000, np.stack([s, s], axis=1).astype(np.float32), R.TRUE_PEAK)
            tp, sp = float(ch.r128()[0]["tp_hold"][0]), float(ch.status()[0]["peak_hold"][0])
            assert tp >= sp and 20.0 * np.log10(tp / 0.5) <= R.TP_TOL[1], (frac, k, tp)
            worst_tp, worst_sample = min(worst_tp, 20.0 * np.log10(tp / 0.5)), min(worst_sample, 20.0 * np.log10(sp / 0.5))
        print(f"{frac} of Nyquist: true peak at worst {worst_tp:.2f} dB, sample peak at worst {worst_sample:.2f} dB")
        assert worst_tp >= worst_sample


def test_streaming_true_peak_carries_eleven_frames(ref):
    """pieces below, at and above the history's length give the one-call result, and the history is the last 11 frames"""
    rng = np.random.default_rng(21)
    x = (0.3 * rng.standard_normal((777, 2))).astype(np.float32)
    one = ref.run(32000, x, R.TRUE_PEAK)
    ch = ref.channel(32000, R.TRUE_PEAK)
    a = 0
    for m in (1, 10, 11, 12, 743):
        ch.process(x[a:a + m])
        a += m
    assert a == 777
    assert np.array_equal(bits(ch.r128()["tp_hold"]), bits(one.r128()["tp_hold"]))
    assert np.array_equal(bits(ch.history()), bits(x[-11:].T)) and np.array_equal(bits(one.history()), bits(x[-11:].T))
    # the first 11 outputs see zeros before the first frame: a lone unit sample reads the largest tap
    imp = np.zeros((40, 2), np.float32)
    imp[0] = 1.0
    assert ref.run(32000, imp, R.TRUE_PEAK).r128()[0]["tp_hold"][0] == 1.0
    imp[0] = 0.0
    imp[20] = -1.0
    t = R.taps_array(ref.tp_design(32000))
    assert ref.run(32000, imp, R.TRUE_PEAK).r128()[0]["tp_hold"][0] == 1.0 and np.abs(t).max() < 1.0
    # L = 1: no filter, the true peak is the sample peak
    ch = ref.run(192000, x, R.TRUE_PEAK)
    assert np.array_equal(bits(ch.r128()[0]["tp_hold"]), bits(ch.status()[0]["peak_hold"]))


@pytest.fixture(scope="module")
def steps_20_30(ref):
    return ref.run(32000, R.level_steps(32000, (-20.0, -30.0)), R.RANGE)


def test_known_answer_range_of_two_levels(pkg, ref, steps_20_30):
    """20 s at -20 LUFS then 20 s at -30 LUFS: 400 sub-blocks, 371 short-term values (171 + 29 in the transition + 171), LRA 10 +- 1"""
    ch = steps_20_30
    h = ch.range_hist()
    r = ch.r128()[0]
    assert int(ch.status()[0]["subblocks"]) == 400 and int(h.sum()) == 371 and int(r["st_below"]) == 0 and int(r["st_nonfinite"]) == 0
    lra, low, high = ch.loudness_range()
    print("LRA, low, high:", lra, low, high)
    assert abs(lra - 10.0) <= 1.0 and abs(high + 20.0) <= 0.2 and abs(low + 30.0) <= 0.2
    d = pkg.meter_design(32000)
    assert pkg.meter_range(h, d) == (lra, low, high) == R.model_range(h, np.array(d.centre))
    # the true-peak fields of a station without the feature stay 0
    assert not r["tp_call"].any() and not r["tp_hold"].any()


def test_known_answer_range_five_lu_and_the_relative_gate(ref, steps_20_30):
    lra, low, high = ref.run(32000, R.level_steps(32000, (-20.0, -15.0)), R.RANGE).loudness_range()
    print("LRA, low, high:", lra, low, high)
    assert abs(lra - 5.0) <= 1.0 and abs(low + 20.0) <= 0.2 and abs(high + 15.0) <= 0.2
    # 20 s at -60 LUFS behind the two levels lie more than 20 LU under the mean: the result does not move
    ch = ref.run(32000, R.level_steps(32000, (-20.0, -30.0, -60.0)), R.RANGE)
    assert int(ch.range_hist().sum()) == 571
    assert ch.loudness_range() == steps_20_30.loudness_range()


def test_range_edge_cases(pkg, ref):
    d = pkg.meter_design(48000)
    rd = ref.design(48000)
    centre = np.array(d.centre)

    def all_three(h):
        got = pkg.meter_range(h, d)
        assert got == ref.range(h, rd) == R.model_range(h, centre), got
        return got

    h = np.zeros(1000, np.uint32)
    with pytest.raises(pkg.FmdError) as e:
        pkg.meter_range(h, d)
    assert e.value.status == -6 and ref.range(h, rd) is None and R.model_range(h, centre) is None
    for j, k in ((0, 1), (470, 1), (470, 4096), (999, 2), (999, 0xffffffff)):
        h[:] = 0
        h[j] = k
        lra, low, high = all_three(h)
        assert lra == 0.0 and low == high and abs(low - (-70.0 + 0.1 * j + 0.05)) < 1e-9
    # counts near 2^32 in every bin: the sums pass 2^32 and the ranks 2^40
    h[:] = 0xfffffff0
    lra, low, high = all_three(h)
    assert 0.0 < lra <= 99.9 and low < high
    # two plateaus with counts near 2^32: ranks 0.10 (n - 1) and 0.95 (n - 1) fall in the lower and the upper
    h[:] = 0
    h[400] = h[500] = 0xffffffff
    assert all_three(h) == (10.0, -70.0 + 0.1 * 400 + 0.05, -70.0 + 0.1 * 500 + 0.05)
    # 10 % + 1 of the values in the lower bin puts rank r10 there; fewer than 10 % leave it in the upper one
    h[:] = 0
    h[300], h[310] = 11, 89
    assert all_three(h)[0] == 1.0
    h[300], h[310] = 9, 91
    assert all_three(h)[0] == 0.0
    # random histograms: the three implementations agree
    rng = np.random.default_rng(22)
    for _ in range(20):
        h[:] = 0
        idx = rng.integers(0, 1000, 40)
        h[idx] = rng.integers(1, 1000, 40)
        all_three(h)
    with pytest.raises(ValueError):
        pkg.meter_range(h[:999], d)


def test_host_code_under_the_sanitizers(tmp_path):
    """tests/cpp/meter_r128_main.cpp with fmd_meter_design.cpp compiled in, built with -fsanitize=address,undefined (the runtimes linked
    statically: the program needs nothing preloaded) and run directly"""
    exe = tmp_path / "meter_r128_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", f"-I{ROOT / 'include'}", f"-I{csrc}", str(ROOT / "tests" / "cpp" / "meter_r128_main.cpp"),
                    str(csrc / "fmd_meter_design.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
