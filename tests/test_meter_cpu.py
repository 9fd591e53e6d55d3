"""Batched loudness meter, the parts that need no GPU: the ABI is declared and exported, the design against BS.1770's printed table, the C
restatement (tests/cpp/meter_ref.c) against a float64 model bit for bit and against the library's own design and read-out, the read-out's
edge cases, and the known answers of EBU Tech 3341 through the restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import meter_ref
from meter_ref import bits

SYMBOLS = ["fmd_meter_design", "fmd_meter_lufs", "fmd_meter_integrated", "fmd_meter_momentary", "fmd_meter_short_term", "fmd_meter_create",
           "fmd_meter_destroy", "fmd_meter_reset", "fmd_meter_reset_peaks", "fmd_meter_process_f32_dev", "fmd_meter_get_status",
           "fmd_meter_get_histogram", "fmd_meter_status_dev", "fmd_meter_last_error"]
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
BS1770_PRE_B = [1.53512485958697, -2.69169618940638, 1.19839281085285]
BS1770_PRE_A = [1.0, -1.69065929318241, 0.73248077421585]
BS1770_RLB_B = [1.0, -2.0, 1.0]
BS1770_RLB_A = [1.0, -1.99004745483398, 0.99007225036621]


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return meter_ref.build(tmp_path_factory.mktemp("meter_ref"))


def test_symbols_are_declared_and_exported(pkg):
    declared = pkg.declared_symbols(debug=False)
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/fmdemod.h"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.fmd_api_version() == 3
    for name in ("LoudnessMeter", "meter_design", "meter_integrated", "METER_STATUS_DTYPE"):
        assert hasattr(pkg, name)
    assert pkg.METER_STATUS_DTYPE == meter_ref.STATUS_DTYPE and pkg.METER_STATUS_DTYPE.itemsize == 280


def test_design(pkg, ref):
    d = pkg.meter_design(48000)
    for got, want in ((d.pre_b, BS1770_PRE_B), (d.pre_a, BS1770_PRE_A), (d.rlb_b, BS1770_RLB_B), (d.rlb_a, BS1770_RLB_A)):
        assert np.max(np.abs(np.array(got) - np.array(want))) <= 1e-12, (list(got), want)
    assert d.frames_per_subblock == 4800
    edge, centre = np.array(d.edge), np.array(d.centre)
    assert edge.shape == (1001,) and centre.shape == (1000,)
    assert (np.diff(edge) > 0).all()
    assert (centre > edge[:-1]).all() and (centre < edge[1:]).all()
    assert abs(pkg.meter_lufs(edge[0]) + 70.0) < 1e-9 and abs(pkg.meter_lufs(edge[1000]) - 30.0) < 1e-9
    for fs in (0, 44101, 7990, 192010, -48000):
        with pytest.raises(pkg.FmdError) as e:
            pkg.meter_design(fs)
        assert e.value.status == -1, fs
    # the library's design, the restatement's and the model's are the same numbers at every rate the tests use
    for fs in (8000, 32000, 44100, 48000, 192000):
        d, r, m = pkg.meter_design(fs), ref.design(fs), meter_ref.model_design(fs)
        assert d.frames_per_subblock == r.nsb == m["nsb"] == fs // 10
        for k in ("pre_b", "pre_a", "rlb_b", "rlb_a", "edge", "centre"):
            a = np.array(getattr(d, k))
            assert np.array_equal(bits(a), bits(np.array(getattr(r, k)))), (fs, k)
            assert np.array_equal(bits(a), bits(np.array(m[k]))), (fs, k)


def test_restatement_equals_the_float64_model_bit_for_bit(ref):
    """3 Nsb + 777 frames of noise at 32 kHz, and the same signal continued by five quieter sub-blocks so that gating blocks exist on
    both sides of the absolute gate (the model runs once: the first case is a prefix of the second)."""
    fs = 32000
    nsb = fs // 10
    n = 3 * nsb + 777
    rng = np.random.default_rng(3)
    x = (0.2 * rng.standard_normal((n, 2))).astype(np.float32)
    x[:, 1] *= np.float32(0.5)
    x = np.concatenate([x, np.tile(x, (2, 1))[: 5 * nsb] * np.float32(1e-4)])
    m = meter_ref.model_run(fs, x)
    st = ref.run(fs, x[:n]).status()[0]
    assert int(st["subblocks"]) == 3 and int(st["frames"]) == n
    assert np.array_equal(bits(st["energy_ring"][:3]), bits(m["energies"][:3])) and not st["energy_ring"][3:].any()
    assert np.array_equal(bits(st["peak_hold"]), bits(np.abs(x[:n]).max(0))) and np.array_equal(bits(st["peak_call"]), bits(st["peak_hold"]))
    ch = ref.run(fs, x)
    st = ch.status()[0]
    G = int(st["subblocks"])
    assert G == 8 and int(st["frames"]) == x.shape[0]
    assert np.array_equal(bits(st["energy_ring"][:G]), bits(m["energies"])) and not st["energy_ring"][G:].any()
    assert np.array_equal(ch.hist(), m["hist"]) and int(ch.hist().sum()) + int(st["below_gate"]) == G - 3
    assert int(st["below_gate"]) == m["below_gate"] and int(st["nonfinite"]) == 0
    assert ch.hist().sum() >= 2 and st["below_gate"] >= 1                       # both outcomes of the absolute gate occur
    assert np.array_equal(bits(st["peak_hold"]), bits(m["peak"])) and np.array_equal(bits(st["peak_call"]), bits(m["peak"]))


def test_library_read_out_equals_the_restatement(pkg, ref):
    rng = np.random.default_rng(4)
    fs = 8000
    x = (rng.standard_normal((35 * 800 + 5, 2)) * np.logspace(-4, -0.5, 35 * 800 + 5)[:, None]).astype(np.float32)
    ch = ref.run(fs, x)
    st, hist = ch.status(), ch.hist()
    d = pkg.meter_design(fs)
    for got, want in ((pkg.meter_momentary(st), ch.momentary()), (pkg.meter_short_term(st), ch.short_term()),
                      (pkg.meter_integrated(hist, d), ch.integrated())):
        assert math.isfinite(want) and np.array_equal(bits(np.float64(got)), bits(np.float64(want))), (got, want)
    for e in (0.0, 1e-300, 5e-324, 1.0, 3.7, np.inf):
        assert np.array_equal(bits(np.float64(pkg.meter_lufs(e))), bits(np.float64(ref.lib.meter_ref_lufs(e))))
    assert pkg.meter_lufs(0.0) == -np.inf and pkg.meter_lufs(1.0) == -0.691


def test_integrated_edge_cases(pkg):
    d = pkg.meter_design(48000)
    centre = np.array(d.centre)
    hist = np.zeros(1000, np.uint32)
    assert pkg.meter_integrated(hist, d) == -np.inf
    # a single bin gives its centre, whatever the count (counts that are powers of two keep count * centre / count exact)
    for j, k in ((0, 1), (470, 1), (470, 4096), (999, 2)):
        hist[:] = 0
        hist[j] = k
        got = pkg.meter_integrated(hist, d)
        assert got == pkg.meter_lufs(centre[j])
        assert abs(got - (-70.0 + 0.1 * j + 0.05)) < 1e-9
    # two populations 17 LU apart, equal counts: Gamma is about half the upper centre, the gate a twentieth of it, the lower centre a
    # fiftieth: dropped, and the result is the upper centre exactly
    hist[:] = 0
    hist[470] = hist[300] = 8
    assert pkg.meter_integrated(hist, d) == pkg.meter_lufs(centre[470])
    # 9 LU apart both stay: the mean of the two centres
    hist[:] = 0
    hist[470] = hist[380] = 8
    assert pkg.meter_integrated(hist, d) == pkg.meter_lufs((8.0 * centre[380] + 8.0 * centre[470]) / 16.0)
    # the windows need their sub-blocks
    st = np.zeros(1, pkg.METER_STATUS_DTYPE)
    st["energy_ring"] = 0.01
    for G, fn, ok in ((0, pkg.meter_momentary, False), (3, pkg.meter_momentary, False), (4, pkg.meter_momentary, True),
                      (29, pkg.meter_short_term, False), (30, pkg.meter_short_term, True), (31, pkg.meter_short_term, True)):
        st["subblocks"] = G
        if ok:
            assert abs(fn(st) - pkg.meter_lufs(0.01)) < 1e-12
        else:
            with pytest.raises(pkg.FmdError) as e:
                fn(st)
            assert e.value.status == -6                                          # FMD_ERR_STATE
    # the ring is read modulo 30: momentary at G = 31 is sub-blocks 27 ... 30, the last of them at slot 0
    st["energy_ring"] = 0.0
    st["energy_ring"][0, 0] = 0.5
    st["subblocks"] = 31
    assert pkg.meter_momentary(st) == pkg.meter_lufs(0.125)


def test_create_without_a_device_or_with_bad_arguments(pkg):
    lib = pkg.load_library()
    h = C.c_void_p()
    for cfg in (pkg.MeterConfig(0, 48000, 1024, -1), pkg.MeterConfig(4, 44101, 1024, -1), pkg.MeterConfig(4, 48000, 0, -1),
                pkg.MeterConfig(4, 7990, 1024, -1), pkg.MeterConfig(4, 48000, (1 << 30) + 1, -1)):
        assert lib.fmd_meter_create(C.byref(cfg), C.byref(h)) == -1              # FMD_ERR_ARG before a device is touched
        assert not h.value and lib.fmd_meter_last_error(None)
    assert lib.fmd_meter_create(None, C.byref(h)) == -1
    if lib.fmd_device_count() <= 0:
        cfg = pkg.MeterConfig(4, 48000, 1024, -1)
        assert lib.fmd_meter_create(C.byref(cfg), C.byref(h)) == -4              # FMD_ERR_NO_DEVICE
        with pytest.raises(pkg.FmdError) as e:
            pkg.LoudnessMeter(4, 48000)
        assert e.value.status == -4


@pytest.mark.parametrize("fs", [32000, 44100, 48000])
def test_known_answer_stereo_sine_at_minus_23_dbfs(ref, fs):
    """EBU Tech 3341 case 1 in spirit: a stereo 1 kHz sine at -23 dBFS per rail reads -23.0 +- 0.1 LU on all three meters.  The float64
    filter alone gives -22.979 (32 kHz), -22.991 (44.1 kHz), -22.993 (48 kHz): the bin centre -22.95 is what the histogram reports."""
    ch = ref.run(fs, meter_ref.sine(fs, 5.0, 1000.0, -23.0, -23.0))
    st = ch.status()[0]
    assert int(st["subblocks"]) == 50 and int(st["below_gate"]) == 0 and int(st["nonfinite"]) == 0
    print(fs, ch.integrated(), ch.momentary(), ch.short_term())
    for v in (ch.integrated(), ch.momentary(), ch.short_term()):
        assert abs(v + 23.0) <= 0.1, v
    assert abs(ch.integrated() + 22.95) < 1e-9
    peak = np.float32(10.0 ** (-23.0 / 20.0))
    assert np.all(st["peak_hold"] <= peak) and np.all(st["peak_hold"] > peak * np.float32(0.99))


def test_known_answer_full_scale_sine_on_one_rail(ref):
    ch = ref.run(48000, meter_ref.sine(48000, 5.0, 997.0, 0.0, None))
    print(ch.integrated(), ch.momentary(), ch.short_term())
    for v in (ch.integrated(), ch.momentary(), ch.short_term()):
        assert abs(v + 3.01) <= 0.1, v
    st = ch.status()[0]
    assert st["peak_hold"][1] == 0.0 and 0.999 < st["peak_hold"][0] <= 1.0
