"""Carrier squelch, the parts that need no GPU: the ABI is declared and exported, the C restatement (tests/cpp/squelch_ref.c) against a
float64 model bit for bit and against the library's own host-only unit, the restatement's split invariance and a sample count past 2^32,
parameter validation, the read-out's edge cases, the gate sequence, known answers, and the host-only unit under sanitizers."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import squelch_ref
import synth
from squelch_ref import bits

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["fmd_squelch_default_params", "fmd_squelch_threshold", "fmd_squelch_level_db", "fmd_squelch_cnr_db", "fmd_squelch_powers",
           "fmd_squelch_create", "fmd_squelch_destroy", "fmd_squelch_reset", "fmd_squelch_reset_peaks", "fmd_squelch_set_params",
           "fmd_squelch_get_params", "fmd_squelch_process_cf32_dev", "fmd_squelch_process_u8_dev", "fmd_squelch_get_status",
           "fmd_squelch_status_dev", "fmd_squelch_last_error"]
# |cnr_db - truth| in dB of synth.fm_capture_realistic (seed 31, 20 intervals, cf32 at amplitude 100) in float64 on the CPU, per rate and
# true CNR: (the worst single interval with window = 1, all twenty with window = 20).  Measured with squelch_ref.model_cnr_db over plain
# float64 sums (see test_known_answers, which prints them); the assertions allow twice these.
KNOWN_ERR = {
    192000: {0: (0.5136, 0.0017), 6: (0.1422, 0.0015), 10: (0.0936, 0.0027), 20: (0.0833, 0.0036), 40: (0.0801, 0.0037)},
    256000: {0: (0.4158, 0.0543), 6: (0.2047, 0.0081), 10: (0.1529, 0.0017), 20: (0.1273, 0.0104), 40: (0.1272, 0.0135)},
    384000: {0: (0.3484, 0.0135), 6: (0.1270, 0.0043), 10: (0.0920, 0.0075), 20: (0.0869, 0.0104), 40: (0.0871, 0.0114)},
}
FS = 192000
M = FS // 20


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return squelch_ref.build(tmp_path_factory.mktemp("squelch_ref"))


@pytest.fixture(scope="module")
def gate_x():
    """the gate sequence at 192 kSa/s as cf32 at amplitude 100 ([n, 2] float32)"""
    return squelch_ref.gate_signal(FS, 100.0).astype(np.float32)


def test_symbols_are_declared_and_exported(pkg):
    declared = pkg.declared_symbols(debug=False)
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/fmdemod.h"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.fmd_api_version() == 3
    for name in ("Squelch", "SquelchConfig", "SquelchParams", "SQUELCH_STATUS_DTYPE", "squelch_default_params", "squelch_threshold",
                 "squelch_level_db", "squelch_cnr_db", "squelch_powers"):
        assert hasattr(pkg, name)
    assert pkg.SQUELCH_STATUS_DTYPE == squelch_ref.STATUS_DTYPE and pkg.SQUELCH_STATUS_DTYPE.itemsize == 368
    assert C.sizeof(pkg.SquelchParams) == C.sizeof(squelch_ref.Params) == 40
    assert (pkg.FMD_SQUELCH_AUTO, pkg.FMD_SQUELCH_FORCE_OPEN, pkg.FMD_SQUELCH_FORCE_CLOSED) == (0, 1, 2)


def test_restatement_equals_the_float64_model_bit_for_bit(ref, gate_x):
    """the whole gate sequence, 23 intervals and 777 samples: every interval's S2, S4 and peak (through the ring, which wraps), the gate
    and its run after every interval, the counters, the held peak and the open interval's partials and peak"""
    mo = squelch_ref.model_run(FS, gate_x, **squelch_ref.GATE_PARAMS)
    ch = ref.channel(FS)
    assert ch.set_params(**squelch_ref.GATE_PARAMS) == 0
    assert len(mo["intervals"]) == 23
    for g, iv in enumerate(mo["intervals"]):
        ch.process(gate_x[g * M:(g + 1) * M])
        st = ch.status()[0]
        assert int(st["intervals"]) == g + 1 and int(st["samples"]) == (g + 1) * M
        for f, want in (("ring_s2", iv["S2"]), ("ring_s4", iv["S4"])):
            assert np.array_equal(bits(st[f][g % 20]), bits(np.float64(want))), (g, f, st[f][g % 20], want)
        assert np.array_equal(bits(st["last_peak"]), bits(np.float32(iv["pk"]))), g
        assert (int(st["open"]), int(st["run"]), ch.mask) == (int(iv["open"]), iv["run"], int(iv["open"])), g
        assert ch.cnr_db(1) == iv["cnr_db"], g
    ch.process(gate_x[23 * M:])
    st = ch.status()[0]
    assert (int(st["transitions"]), int(st["intervals_open"]), int(st["nonfinite"])) == (mo["transitions"], mo["intervals_open"], 0)
    assert int(st["samples"]) == gate_x.shape[0] and int(st["intervals"]) == 23
    assert np.array_equal(bits(st["hold_peak"]), bits(np.float32(mo["hold_peak"]))) and np.array_equal(bits(np.float32(ch.c.pk)), bits(np.float32(mo["pk"])))
    assert np.array_equal(bits(np.ctypeslib.as_array(ch.c.p)), bits(np.array(mo["part"], np.float64)))
    assert ref.threshold(10.0) == squelch_ref.model_threshold(10.0) and ref.threshold(7.0) == squelch_ref.model_threshold(7.0)
    # the read-out over twenty intervals of the ring, oldest first
    assert ch.cnr_db(20) == squelch_ref.model_cnr_db([mo["intervals"][g]["S2"] for g in range(3, 23)], [mo["intervals"][g]["S4"] for g in range(3, 23)], M)


def test_library_host_unit_equals_the_restatement(pkg, ref, gate_x):
    """threshold, default parameters and the three read-outs: the same bits"""
    for db in (0.0, 0.5, 3.0, 7.0, 8.5, 10.0, 20.0, 33.3, 60.0, -3.0, 100.0):
        assert np.array_equal(bits(np.float64(pkg.squelch_threshold(db))), bits(np.float64(ref.threshold(db)))), db
    assert abs(pkg.squelch_threshold(10.0) - (10.0 / 11.0) ** 2) < 1e-15 and pkg.squelch_threshold(0.0) == 0.25
    d = pkg.squelch_default_params()
    assert bytes(d) == bytes(ref.default_params())
    assert (d.open_db, d.close_db, d.min_level_db, d.open_intervals, d.close_intervals, d.mode) == (10.0, 7.0, -math.inf, 2, 10, 0)
    ch = ref.channel(FS)
    for g in range(23):
        ch.process(gate_x[g * M:(g + 1) * M])
        st = ch.status()[0]
        assert np.array_equal(bits(np.float64(pkg.squelch_level_db(st, FS))), bits(np.float64(ch.level_db())))
        for w in (1, 2, 7, 20):
            if w > g + 1:
                with pytest.raises(pkg.FmdError) as e:
                    pkg.squelch_cnr_db(st, FS, w)
                assert e.value.status == -6 and ch.cnr_db(w) is None
                continue
            assert np.array_equal(bits(np.float64(pkg.squelch_cnr_db(st, FS, w))), bits(np.float64(ch.cnr_db(w)))), (g, w)
            assert np.array_equal(bits(np.float64(pkg.squelch_powers(st, FS, w))), bits(np.float64(ch.powers(w)))), (g, w)
    # the level is the mean power: a carrier of amplitude 100 in noise 20 dB down
    assert abs(pkg.squelch_level_db(ch.status()[0], FS) - 10.0 * math.log10(100.0 ** 2 * 1.01)) < 0.05
    c, nz = pkg.squelch_powers(ch.status()[0], FS, 1)
    assert abs(10.0 * math.log10(c / nz) - pkg.squelch_cnr_db(ch.status()[0], FS, 1)) < 1e-9 and abs(c - 1e4) < 100.0


def test_readout_edge_cases(pkg, ref):
    fresh = np.zeros(1, squelch_ref.STATUS_DTYPE)
    for fn in (lambda: pkg.squelch_level_db(fresh, 256000), lambda: pkg.squelch_cnr_db(fresh, 256000), lambda: pkg.squelch_powers(fresh, 256000)):
        with pytest.raises(pkg.FmdError) as e:
            fn()
        assert e.value.status == -6                              # intervals < window
    assert ref.readout("squelch_ref_cnr_db", fresh, 256000, 1)[0] == -6 and ref.readout("squelch_ref_level_db", fresh, 256000)[0] == -6
    st = fresh.copy()
    st["intervals"] = 3
    Mm = 12800.0
    # arguments: the rate and the window
    for fn in (lambda: pkg.squelch_cnr_db(st, 1024000), lambda: pkg.squelch_cnr_db(st, 256500), lambda: pkg.squelch_level_db(st, 0),
               lambda: pkg.squelch_cnr_db(st, 256000, 0), lambda: pkg.squelch_cnr_db(st, 256000, 21), lambda: pkg.squelch_powers(st, 256000, -1)):
        with pytest.raises(pkg.FmdError) as e:
            fn()
        assert e.value.status == -1
    with pytest.raises(pkg.FmdError) as e:
        pkg.squelch_cnr_db(st, 256000, 4)
    assert e.value.status == -6
    # d <= 0: -inf.  Silence (d = 0), and noise alone, whose 2 S2^2 - M S4 is negative as often as not
    assert pkg.squelch_cnr_db(st, 256000, 1) == -math.inf and pkg.squelch_level_db(st, 256000) == -math.inf
    st["ring_s2"][0, 2], st["ring_s4"][0, 2] = 100.0 * Mm, 2.0 * 100.0 ** 2 * Mm * 1.001
    assert pkg.squelch_cnr_db(st, 256000, 1) == -math.inf == ref.readout("squelch_ref_cnr_db", st, 256000, 1)[1]
    assert pkg.squelch_powers(st, 256000, 1) == (0.0, 100.0) == squelch_ref.ref_powers(ref.lib, st, 256000, 1)[1:]
    # nz <= 0: +inf.  A carrier and nothing else
    st["ring_s2"][0, 2], st["ring_s4"][0, 2] = 64.0 * Mm, 64.0 ** 2 * Mm
    assert pkg.squelch_cnr_db(st, 256000, 1) == math.inf == ref.readout("squelch_ref_cnr_db", st, 256000, 1)[1]
    assert pkg.squelch_powers(st, 256000, 1) == (64.0, 0.0) and pkg.squelch_level_db(st, 256000) == 10.0 * math.log10(64.0)
    # the window reaches back over the two silent intervals before it: an envelope that is there a third of the time is no carrier
    assert pkg.squelch_cnr_db(st, 256000, 3) == -math.inf == ref.readout("squelch_ref_cnr_db", st, 256000, 3)[1]
    # ... and over an interval at half the amplitude: a carrier again, its change of level read as noise
    st["ring_s2"][0, 1], st["ring_s4"][0, 1] = 16.0 * Mm, 16.0 ** 2 * Mm
    assert 0.0 < pkg.squelch_cnr_db(st, 256000, 2) < 10.0 and pkg.squelch_cnr_db(st, 256000, 2) == ref.readout("squelch_ref_cnr_db", st, 256000, 2)[1]
    # a non-finite ring entry reads as a NaN (inf - inf in d), in the library and the restatement alike; the level is log10's own
    for bad in (math.inf, math.nan):
        s = st.copy()
        s["ring_s2"][0, 1], s["ring_s4"][0, 1] = bad, bad
        assert math.isnan(pkg.squelch_cnr_db(s, 256000, 2)) and math.isnan(ref.readout("squelch_ref_cnr_db", s, 256000, 2)[1])
        assert all(math.isnan(v) for v in pkg.squelch_powers(s, 256000, 2))
        assert pkg.squelch_cnr_db(s, 256000, 1) == math.inf      # the newest interval alone is clean
        s["intervals"] = 2
        lv = pkg.squelch_level_db(s, 256000)
        assert (lv == math.inf) if bad == math.inf else math.isnan(lv)
    # the ring's index is the interval's number mod 20, in 64 bits
    s = fresh.copy()
    s["intervals"] = (1 << 40) + 7                               # newest at [((1 << 40) + 6) % 20] = [2]
    s["ring_s2"][0, 2], s["ring_s4"][0, 2] = 64.0 * Mm, 64.0 ** 2 * Mm
    assert ((1 << 40) + 6) % 20 == 2 and pkg.squelch_cnr_db(s, 256000, 1) == math.inf and pkg.squelch_level_db(s, 256000) == 10.0 * math.log10(64.0)


def test_parameter_validation(ref):
    """the restatement's checks, which the library's fmd_squelch_set_params shares (tests/test_gpu_squelch.py and the sanitizer program
    below run the library's): a rejected set changes nothing"""
    ch = ref.channel(FS)
    before = bytes(ch.c.prm)
    bad = [dict(open_db=60.5), dict(close_db=-0.1), dict(close_db=10.5), dict(open_db=6.0), dict(open_db=math.nan), dict(close_db=math.nan),
           dict(min_level_db=math.inf), dict(min_level_db=math.nan), dict(open_intervals=0), dict(open_intervals=1001), dict(close_intervals=0),
           dict(close_intervals=1001), dict(mode=3), dict(mode=-1)]
    for b in bad:
        assert ch.set_params(**b) == -1, b
        assert bytes(ch.c.prm) == before and ch.c.c_open == ref.threshold(10.0)
    for ok in (dict(open_db=60.0, close_db=60.0), dict(open_db=0.0, close_db=0.0), dict(open_db=10.0, close_db=7.0, min_level_db=-200.0),
               dict(min_level_db=35.5, open_intervals=1000, close_intervals=1, mode=2)):
        assert ch.set_params(**ok) == 0, ok
    assert ch.c.min_s2 == math.pow(10.0, 3.55) * M and int(ch.status()[0]["mode"]) == 2
    assert ch.set_params(min_level_db=-math.inf) == 0 and ch.c.min_s2 == 0.0 and math.copysign(1.0, ch.c.min_s2) == 1.0
    for fs in (191000, 385000, 1024000, 256500, 0):
        with pytest.raises(ValueError):
            ref.channel(fs)


def test_restatement_split_invariance_u8_and_counts_past_2_32(ref):
    fs = 250000
    Mm = fs // 20                                                # 12500: no multiple of 256
    x = squelch_ref.gate_signal(fs, 100.0, seed=21)[5 * Mm:8 * Mm + 555].astype(np.float32)   # three intervals at 20 dB and a bit
    prm = dict(open_intervals=1, close_intervals=1)
    whole = ref.run(fs, x, **prm)
    ch = ref.channel(fs)
    ch.set_params(**prm)
    a = 0
    for k in (1, 255, 256, 257, Mm - 1, Mm, Mm + 1, 0, x.shape[0]):
        b = min(a + k, x.shape[0])
        ch.process(x[a:b])
        a = b
    assert a == x.shape[0]
    assert np.array_equal(bits(ch.status()), bits(whole.status())) and bytes(ch.c.p) == bytes(whole.c.p) and ch.c.pk == whole.c.pk
    assert int(whole.status()[0]["intervals"]) == 3
    # the bytes of a receiver against their floats
    b8 = squelch_ref.to_u8(0.4 * x)
    assert np.array_equal(bits(ref.run(fs, b8, **prm).status()), bits(ref.run(fs, squelch_ref.from_u8(b8), **prm).status()))
    # a station whose count starts above 2^32, at the start of interval G0: the same sums land G0 slots further round the ring
    G0 = (1 << 33) // Mm + 7
    far = ref.channel(fs)
    far.set_params(**prm)
    far.c.st.samples, far.c.st.intervals = G0 * Mm, G0
    far.process(x[:777]).process(x[777:])
    fs_, ws = far.status()[0], whole.status()[0]
    assert int(fs_["samples"]) == G0 * Mm + x.shape[0] > 1 << 32 and int(fs_["intervals"]) == G0 + 3
    for g in range(3):
        for f in ("ring_s2", "ring_s4"):
            assert np.array_equal(bits(fs_[f][(G0 + g) % 20]), bits(ws[f][g])), (g, f)
    for f in ("last_peak", "hold_peak", "run", "transitions", "open", "intervals_open", "nonfinite"):
        assert fs_[f] == ws[f], f
    assert bytes(far.c.p) == bytes(whole.c.p) and far.cnr_db(3) == whole.cnr_db(3)


@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_gate_sequence(ref, gate_x, fmt):
    """fs = 192000, open_intervals = 2, close_intervals = 3, thresholds 10 / 7 dB; a noise-FM carrier (amplitude 100 as cf32, 40 LSB as u8)
    in complex Gaussian noise: absent x 3, 20 dB x 1 (must not open), absent x 1, 20 dB x 4 (opens at the second), 8.5 dB x 3 (stays open:
    hysteresis), absent x 2 (stays open: hold), 20 dB x 1, absent x 3 (closes at the third), 8.5 dB x 3 (stays closed), 20 dB x 2 (opens
    at the second), 777 samples of an open interval.  The mask after every interval, three transitions; and in float64 no interval reads
    within 1 dB of a threshold it must not cross (seed 5 reads 8.39 ... 8.60 dB, 19.9 ... 20.1 dB and at most -6.0 dB without a carrier)."""
    x = gate_x if fmt == "cf32" else squelch_ref.to_u8(squelch_ref.gate_signal(FS, 40.0))
    seen = gate_x if fmt == "cf32" else squelch_ref.from_u8(x)
    levels = squelch_ref.gate_levels()
    assert squelch_ref.expected_masks(levels, **squelch_ref.GATE_PARAMS) == (squelch_ref.GATE_MASK, 3) and len(levels) == 23
    cnr = squelch_ref.interval_cnr_db(seen, M)
    print(fmt, "float64 cnr_db per interval", [round(v, 2) for v in cnr])
    for g, (lv, v) in enumerate(zip(levels, cnr)):
        if lv is None:
            assert v < 7.0 - 1.0, (g, v)                         # crosses neither threshold
        elif lv == 8.5:
            assert 7.0 + 1.0 < v < 10.0 - 1.0, (g, v)            # inside the hysteresis band
        else:
            assert v > 10.0 + 1.0, (g, v)
    assert float(np.abs(seen).max()) < (127.0 if fmt == "u8" else 1e9)   # the bytes do not reach the rails
    ch = ref.channel(FS)
    assert ch.mask == 0xAA and ch.set_params(**squelch_ref.GATE_PARAMS) == 0
    for g in range(23):
        ch.process(x[g * M:(g + 1) * M])
        assert ch.mask == squelch_ref.GATE_MASK[g] == int(ch.status()[0]["open"]), (fmt, g)
        assert abs(ch.cnr_db(1) - cnr[g]) < 1e-9 or cnr[g] == ch.cnr_db(1)
    ch.process(x[23 * M:])
    st = ch.status()[0]
    assert ch.mask == 1 and int(st["transitions"]) == 3 and int(st["intervals"]) == 23 and int(st["samples"]) == 23 * M + 777
    assert int(st["intervals_open"]) == sum(squelch_ref.GATE_MASK)
    # the modes move the mask byte and nothing else
    before = ch.status()
    for mode, want in ((squelch_ref.FORCE_CLOSED, 0), (squelch_ref.FORCE_OPEN, 1), (squelch_ref.AUTO, 1)):
        ch.set_params(mode=mode)
        ch.process(x[:0])
        assert ch.mask == want
    assert np.array_equal(bits(ch.status()), bits(before))


@pytest.mark.parametrize("fs", [256000, 192000, 384000])
def test_known_answers(pkg, ref, fs):
    """cnr_db of oracle/synth.py's realistic station (twenty intervals as cf32 at amplitude 100) at a true CNR of 0, 6, 10, 20 and 40 dB
    through the restatement and the library's read-out: every interval with window = 1 and all of them with window = 20 within twice
    KNOWN_ERR; the level is the carrier's plus the noise's power."""
    Mm = fs // 20
    for cnr in (0, 6, 10, 20, 40):
        x = synth.to_cf32(synth.fm_capture_realistic(20 * Mm, fs=float(fs), seed=31, cnr_db=float(cnr))["iq"])
        ch = ref.channel(fs)
        w1 = []
        for g in range(20):
            ch.process(x[g * Mm:(g + 1) * Mm])
            w1.append(pkg.squelch_cnr_db(ch.status()[0], fs, 1))
            assert w1[-1] == ch.cnr_db(1)
        w20 = pkg.squelch_cnr_db(ch.status()[0], fs, 20)
        model = squelch_ref.interval_cnr_db(x, Mm)
        err1, err20 = max(abs(v - cnr) for v in w1), abs(w20 - cnr)
        print(fs, cnr, "worst interval", err1, "window 20", err20, "float64 model's worst", max(abs(v - cnr) for v in model))
        assert err1 <= 2.0 * KNOWN_ERR[fs][cnr][0] and err20 <= 2.0 * KNOWN_ERR[fs][cnr][1], (fs, cnr, err1, err20)
        assert abs(pkg.squelch_level_db(ch.status()[0], fs) - 10.0 * math.log10(1e4 * (1.0 + 10.0 ** (-cnr / 10.0)))) < 0.1
        assert int(ch.status()[0]["nonfinite"]) == 0


def test_noise_alone_never_opens_at_0_db(ref):
    """400 intervals of complex Gaussian noise at 256 kSa/s with open_db = close_db = 0 and one interval to open: no interval is
    good_open (the gate never opens); the highest reading in float64 is -5.4 dB"""
    fs = 256000
    z = (100.0 * math.sqrt(0.5) * np.random.default_rng(9).standard_normal((400 * (fs // 20), 2))).astype(np.float32)
    ch = ref.run(fs, z, open_db=0.0, close_db=0.0, open_intervals=1, close_intervals=1)
    st = ch.status()[0]
    assert (int(st["intervals"]), int(st["transitions"]), int(st["intervals_open"]), int(st["open"]), int(st["run"])) == (400, 0, 0, 0, 0)
    cnr = squelch_ref.interval_cnr_db(z, fs // 20)
    print("noise alone: highest reading", max(cnr), "intervals at -inf", sum(v == -math.inf for v in cnr))
    assert max(cnr) < 0.0


def test_host_unit_under_sanitizers(pkg, ref, tmp_path):
    """fmd_squelch_design.cpp and tests/cpp/squelch_design_main.cpp, built with -fsanitize=address,undefined and run as a stand-alone
    program: clean, and the thresholds and default parameters it prints are the library's"""
    exe = tmp_path / "squelch_design_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{csrc}", str(csrc / "fmd_squelch_design.cpp"),
                    str(ROOT / "tests" / "cpp" / "squelch_design_main.cpp"), "-o", str(exe)], check=True)
    dbs = (0.0, 7.0, 8.5, 10.0, 33.3, 60.0)
    r = subprocess.run([str(exe)] + [repr(d) for d in dbs], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split()
    assert lines[-1] == "ok" and lines[-2] == "readout"
    for db, line in zip(dbs, lines):
        assert bytes.fromhex(line) == np.float64(pkg.squelch_threshold(db)).tobytes(), db
    assert bytes.fromhex(lines[len(dbs)]) == bytes(pkg.squelch_default_params())
