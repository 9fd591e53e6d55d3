"""Look-ahead peak limiter, the parts that need no GPU: the C restatement (tests/cpp/limiter_ref.c) against a numpy restatement written
the other way, bit for bit; the ceiling and the transparent delay as properties; the restatement's split invariance; that the signals
of the GPU comparison reach the limiter's every path; the library's host-only functions against the header's formulas, at their
bounds; and the host-only unit as a stand-alone program under sanitizers."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import limiter_ref as R
from limiter_ref import ONE, bits

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["fmd_limiter_design", "fmd_limiter_default_config", "fmd_limiter_gain_for_loudness", "fmd_limiter_create", "fmd_limiter_destroy", "fmd_limiter_reset",
           "fmd_limiter_set_gain", "fmd_limiter_get_gain", "fmd_limiter_process_f32_dev", "fmd_limiter_flush", "fmd_limiter_get_status", "fmd_limiter_status_dev",
           "fmd_limiter_last_error"]
CONFIGS = [(D, step) for D in R.DS for step in R.STEPS]


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("limiter_ref"))


def _stream(D: int, gain: float, seed: int = 0) -> np.ndarray:
    W = D + 1
    return R.signal(R.stream_length(W), gain, R.ceiling(), W, seed=100 * D + seed)


def _same_record(st, m, frames=None):
    """a restatement's status record against the numpy restatement's counters"""
    assert int(st["frames"][0]) == (m["frames"] if frames is None else frames)
    assert int(st["limited"][0]) == m["limited"] and st["clamped"][0].tolist() == m["clamped"] and int(st["nonfinite"][0]) == m["nonfinite"]
    assert bits(st["min_gain"]).tolist() == bits(m["min_gain"]).tolist() and int(st["eq"][0]) == m["eq_last"]


def test_symbols_are_declared_and_exported(pkg):
    declared = pkg.declared_symbols(debug=False)
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/fmdemod.h"
        assert hasattr(lib, s), f"{s} is not exported"
    assert "fmd_limiter_debug_set_frames" not in pkg.declared_symbols() and hasattr(lib, "fmd_limiter_debug_set_frames") and lib.fmd_api_version() == 3
    for name in ("Limiter", "LimiterConfig", "LimiterDesign", "LIMITER_STATUS_DTYPE", "limiter_design", "limiter_default_config", "limiter_gain_for_loudness"):
        assert hasattr(pkg, name)
    assert pkg.LIMITER_STATUS_DTYPE == R.STATUS_DTYPE and pkg.LIMITER_STATUS_DTYPE.itemsize == 64
    assert [pkg.LIMITER_STATUS_DTYPE.fields[k][1] for k in ("frames", "limited", "clamped", "nonfinite", "min_gain", "gain", "eq", "reserved")] == [0, 8, 16, 32, 40, 44, 48, 52]


@pytest.mark.parametrize("D,step", CONFIGS)
def test_restatement_equals_numpy(ref, D, step):
    """The sequential restatement and the vectorised one agree bit for bit on the output, the flush's frames, eq along the stream (read
    behind every piece of a ragged split) and every counter, for each gain"""
    T = R.ceiling()
    for k, gain in enumerate(R.GAINS):
        x = _stream(D, gain, k)
        m = R.numpy_limiter(x, gain, D, step, T, flush=True)
        ch = ref.channel(D, step, T, gain)
        ys, at = [], 0
        for piece in [1, 2, 3, D, D + 1, 7, 300, 1024, 1, 10 ** 9]:
            y, g = ch.process(x[at:at + piece])
            take = y.shape[0]
            ys.append(y)
            if take:
                assert ch.eq == int(m["eq"][at + take - 1]), (gain, at)
                assert bits(g).tolist() == bits(m["g"][at:at + take].min()).tolist(), (gain, at)
            at += take
        assert at == x.shape[0]
        ys.append(ch.flush())
        y = np.concatenate(ys)
        assert y.shape[0] == x.shape[0] + D
        assert np.array_equal(bits(y), bits(m["y"])), gain
        _same_record(ch.status(), m)
        assert float(ch.status()["gain"][0]) == float(np.float32(gain))


def test_eq_frame_by_frame(ref):
    """eq behind every single frame, at the middle configuration"""
    D, step, gain, T = 47, 6711, 1.7, R.ceiling()
    x = _stream(D, gain)[:1500]
    m = R.numpy_limiter(x, gain, D, step, T)
    ch = ref.channel(D, step, T, gain)
    for n in range(x.shape[0]):
        y, _ = ch.process(x[n:n + 1])
        assert ch.eq == int(m["eq"][n]) and bits(y).tolist() == bits(m["y"][n:n + 1]).tolist(), n
    assert m["limited"] > 0 and (m["eq"] < ONE).any() and (m["eq"] == ONE).any()


@pytest.mark.parametrize("D,step", CONFIGS)
def test_ceiling_and_transparent_delay(ref, D, step):
    """|y| <= T on every sample; and where no frame in [n - 2D, n] exceeds T after the gain and eq stood at ONE just before that window's
    last W frames, y[n] is u[n - D] bit for bit"""
    T = R.ceiling()
    W = D + 1
    for k, gain in enumerate(R.GAINS):
        x = _stream(D, gain, k)
        ch = ref.channel(D, step, T, gain)
        y, _ = ch.process(x)
        assert np.isfinite(y).all() and float(np.abs(y).max()) <= float(T)
        u, _ = R.gained(x, gain)
        n = x.shape[0]
        over = np.concatenate([np.zeros(2 * D, bool), np.max(np.abs(u), axis=1) > T])
        clean = ~np.lib.stride_tricks.sliding_window_view(over, 2 * D + 1).any(axis=1)        # [n]: nothing over T in [n - 2D, n]
        eq = np.concatenate([np.full(W, ONE, np.int64), R.numpy_limiter(x, gain, D, step, T)["eq"]])
        recovered = eq[:n] == ONE                                                              # eq[n - D - 1]
        where = clean & recovered
        ud = np.concatenate([np.zeros((D, 2), np.float32), u])[:n]
        assert where[:5 * W + 10].all() and where.sum() >= 4 * W
        assert np.array_equal(bits(y[where]), bits(ud[where])), gain


def test_rounding_cases(ref):
    """T / p and the conversion, on known answers: at the ceiling, an ulp above it, twice it, and where the quotient is a denormal"""
    T = R.ceiling()
    assert ref.rq(float(T), 0.0, T) == ONE and ref.rq(0.0, -float(T), T) == ONE and ref.rq(0.0, 0.0, T) == ONE
    up = np.nextafter(T, np.float32(2.0))
    assert ref.rq(float(up), 0.0, T) == int(np.float32(T / up) * np.float32(ONE)) < ONE
    assert ref.rq(0.1, float(2 * T), T) == ONE // 2
    assert ref.rq(3e38, 0.0, T) == 0 and np.float32(T / np.float32(3e38)) > 0                  # a denormal quotient, kept, truncates to 0
    assert ref.rq(3.0, 0.0, np.float32(1.0)) == int(np.float32(np.float32(1.0) / np.float32(3.0)) * np.float32(ONE)) == 357913952


def test_split_invariance(ref):
    """however the stream is cut into calls, gains set between calls included, the restatement gives the same bits"""
    T = R.ceiling()
    for D, step in ((0, 6711), (1, 1), (47, 6711), (255, ONE)):
        x = _stream(D, 1.7)
        half = x.shape[0] // 2
        whole = ref.channel(D, step, T, 1.7)
        y0a, _ = whole.process(x[:half])
        whole.set_gain(0.9)
        y0b, _ = whole.process(x[half:])
        y0 = np.concatenate([y0a, y0b, whole.flush()])
        rng = np.random.default_rng(D)
        for trial in range(3):
            ch = ref.channel(D, step, T, 1.7)
            cuts = np.sort(rng.integers(0, half, 40)) if trial else np.arange(0, half, 1)
            edges = [0, *cuts.tolist(), half]
            ys = [ch.process(x[a:b])[0] for a, b in zip(edges[:-1], edges[1:])]
            ch.set_gain(0.9)
            ys += [ch.process(x[half:half + 3])[0], ch.process(x[half + 3:])[0], ch.flush()]
            assert np.array_equal(bits(np.concatenate(ys)), bits(y0)), (D, step, trial)
            assert ch.status().tobytes() == whole.status().tobytes()


def test_reset_and_flush(ref):
    """a flush leaves the signal state of a reset and keeps counters and gain; a reset clears the counters and keeps the gain; a flush right
    after either writes D zero frames at unity"""
    D, step, T = 47, 6711, R.ceiling()
    x = _stream(D, 4.0)
    ch = ref.channel(D, step, T, 4.0)
    first, _ = ch.process(x[:900])
    tail = ch.flush()
    st = ch.status()
    assert int(st["frames"][0]) == 900 and int(st["eq"][0]) == ONE and float(st["gain"][0]) == 4.0 and int(st["limited"][0]) > 0
    assert not ch.flush().any() and ch.status().tobytes() == st.tobytes()                     # flush twice: zeros, nothing moves
    again, _ = ch.process(x[:900])
    assert np.array_equal(bits(again), bits(first)) and np.array_equal(bits(ch.flush()), bits(tail))
    ch.reset()
    st = ch.status()
    assert int(st["frames"][0]) == 0 and int(st["limited"][0]) == 0 and float(st["min_gain"][0]) == 1.0 and float(st["gain"][0]) == 4.0
    assert not ch.flush().any()


def test_gpu_signals_reach_every_path(ref):
    """What tests/test_gpu_limiter.py compares is worth comparing: on its signals the restatement alone limits (limited > 0) at every
    configuration, clamps (clamped > 0) on at least one, counts the non-finite samples, and leaves a transparent stretch of 4W frames"""
    T = R.ceiling()
    clamped = 0
    for D, step in CONFIGS:
        W = D + 1
        for gain, x in zip(R.GAINS, R.gpu_streams(D)):                                        # that test's own streams
            ch = ref.channel(D, step, T, gain)
            y, _ = ch.process(x)
            st = ch.status()
            assert int(st["limited"][0]) > 0 and int(st["nonfinite"][0]) >= 4 and float(st["min_gain"][0]) < 0.1
            clamped += int(st["clamped"][0].sum())
            u, _ = R.gained(x, gain)
            assert np.array_equal(bits(y[D:5 * W + 10]), bits(u[:5 * W + 10 - D]))           #the first 5W + 10 frames: the delayed input itself
            if gain in (0.5, 4.0):                                                            # (powers of two: the products are exact)
                xt = R.exact_at(T, gain)
                assert np.float32(xt * np.float32(gain)) == T and np.float32(np.nextafter(xt, np.float32(2.0)) * np.float32(gain)) > T
    assert clamped > 0


def test_design_formulas_and_bounds(pkg):
    for fs, la, rel, db in ((32000, 1.5, 500.0, -1.0), (48000, 2.0, 120.0, -0.3), (8000, 0.0, 0.0, 0.0), (192000, 1.0, 3.5, -40.0), (44100, 5.78, 1e4, -6.0)):
        d = pkg.limiter_design(fs, la, rel, db)
        frames = rel * fs / 1000.0
        step = ONE if frames == 0 else min(max(int(math.floor(ONE / frames + 0.5)), 1), ONE)
        assert d.lookahead_frames == d.latency_frames == int(math.floor(la * fs / 1000.0 + 0.5))
        assert d.step == step and bits(np.float32(d.ceiling)).tolist() == bits(np.float32(10.0 ** (db / 20.0))).tolist()
    # D = 0 and 255; 256 refused
    assert pkg.limiter_design(32000, 0.0, 500.0, -1.0).lookahead_frames == 0
    assert pkg.limiter_design(32000, 255.0 / 32.0, 500.0, -1.0).lookahead_frames == 255
    with pytest.raises(pkg.FmdError):
        pkg.limiter_design(32000, 256.0 / 32.0, 500.0, -1.0)
    # step at 1 and at 2^30
    assert pkg.limiter_design(32000, 1.5, 0.0, -1.0).step == ONE
    assert pkg.limiter_design(32000, 1.5, 1.0 / 64.0, -1.0).step == ONE                        # half a frame: clamped
    assert pkg.limiter_design(32000, 1.5, float(ONE) / 32.0, -1.0).step == 1
    assert pkg.limiter_design(32000, 1.5, 1e11, -1.0).step == 1                                # clamped from 0
    assert pkg.limiter_design(32000, 1.5, 5000.0, -1.0).step == 6711
    # ceiling 0 and -40 dB
    assert pkg.limiter_design(32000, 1.5, 500.0, 0.0).ceiling == 1.0
    assert bits(np.float32(pkg.limiter_design(32000, 1.5, 500.0, -40.0).ceiling)).tolist() == bits(np.float32(0.01)).tolist()
    for bad in ((7999, 1.5, 500.0, -1.0), (192001, 1.5, 500.0, -1.0), (32000, -0.1, 500.0, -1.0), (32000, 1.5, -1.0, -1.0), (32000, 1.5, 500.0, 0.1),
                (32000, 1.5, 500.0, -40.1), (32000, float("nan"), 500.0, -1.0), (32000, 1.5, float("nan"), -1.0), (32000, 1.5, 500.0, float("nan"))):
        with pytest.raises(pkg.FmdError):
            pkg.limiter_design(*bad)
    lib = pkg.load_library()
    assert lib.fmd_limiter_design(32000, 1.5, 500.0, -1.0, None) == -1 and b"null" in lib.fmd_limiter_last_error(None)
    # the GPU comparison's milliseconds design to its (D, step)
    for D in R.DS:
        for step in R.STEPS:
            d = pkg.limiter_design(R.FS, R.LOOKAHEAD_MS[D], R.RELEASE_MS[step], R.CEILING_DB)
            assert (d.lookahead_frames, d.step) == (D, step) and np.float32(d.ceiling) == R.ceiling()


def test_defaults_and_gain_helper(pkg):
    cfg = pkg.limiter_default_config(32000)
    assert (cfg.n_channels, cfg.fs, cfg.lookahead_ms, cfg.release_ms, cfg.ceiling_db, cfg.max_input_frames, cfg.device) == (1, 32000, 1.5, 500.0, -1.0, 65536, -1)
    d = pkg.limiter_design(cfg.fs, cfg.lookahead_ms, cfg.release_ms, cfg.ceiling_db)
    assert (d.lookahead_frames, d.step) == (48, 67109)
    # a 3 dB reduction recovers in about 150 ms
    assert 140.0 < (1.0 - 10.0 ** (-3.0 / 20.0)) * ONE / d.step / 32.0 < 160.0
    with pytest.raises(pkg.FmdError):
        pkg.limiter_default_config(7000)
    assert C.sizeof(pkg.LimiterConfig) == 48 and pkg.LimiterConfig.max_input_frames.offset == 32 and pkg.LimiterConfig.device.offset == 40
    for lufs, target in ((-23.0, -23.0), (-17.3, -23.0), (-31.0, -16.0), (-70.0, -23.0)):
        assert bits(np.float32(pkg.limiter_gain_for_loudness(lufs, target))).tolist() == bits(np.float32(10.0 ** ((target - lufs) / 20.0))).tolist()
    assert pkg.limiter_gain_for_loudness(-23.0) == 1.0 and pkg.limiter_gain_for_loudness(float("-inf")) == float("inf")


def test_create_refuses_bad_configurations_before_any_device_work(pkg):
    """the argument checks come first: they answer alike with and without a GPU"""
    lib = pkg.load_library()
    h = C.c_void_p()
    for fields in ({"n_channels": 0}, {"max_input_frames": 0}, {"max_input_frames": (1 << 30) + 1}, {"lookahead_ms": 8.0}, {"ceiling_db": 1.0}, {"fs": 1000}):
        cfg = pkg.limiter_default_config(32000)
        for k, v in fields.items():
            setattr(cfg, k, v)
        assert lib.fmd_limiter_create(C.byref(cfg), C.byref(h)) == -1 and lib.fmd_limiter_last_error(None), fields
    assert lib.fmd_limiter_create(None, C.byref(h)) == -1


def test_host_unit_under_sanitizers(tmp_path):
    """fmd_limiter_design.cpp and tests/cpp/limiter_design_main.cpp, built with -fsanitize=address,undefined and run as a stand-alone
    program: clean; the design at its bounds, and the process call's checks (the overlap of the two ranges among them) with each bound
    held from both sides"""
    exe = tmp_path / "limiter_design_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{csrc}", str(csrc / "fmd_limiter_design.cpp"),
                    str(ROOT / "tests" / "cpp" / "limiter_design_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True)
    assert out.stdout.strip() == "ok" and not out.stderr
