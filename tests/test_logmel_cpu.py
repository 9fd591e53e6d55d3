"""Log-mel front end without a GPU (fmd_logmel_*, include/fmdemod.h "Log-mel front end"): the C restatement of the arithmetic contract
(tests/cpp/logmel_ref.c) against an independent float64 definition by an a-priori bound, its framing against torch.stft, the mel
filterbank's known answers, flog10's 8 ulp condition, the restatement's split invariance, the library's host-only functions against the
restatement, and the host-only unit as a stand-alone program under sanitizers."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import logmel_ref
from logmel_ref import bits

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["fmd_logmel_default_config", "fmd_logmel_design", "fmd_logmel_bins", "fmd_logmel_max_frames", "fmd_logmel_flog10", "fmd_logmel_create",
           "fmd_logmel_destroy", "fmd_logmel_reset", "fmd_logmel_process_f32_dev", "fmd_logmel_get_status", "fmd_logmel_status_dev", "fmd_logmel_last_error"]
SIGNALS = ("noise", "tone", "tone_noise")


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return logmel_ref.build(tmp_path_factory.mktemp("logmel_ref"))


def _lib_config(pkg, cfg):
    """the library's LogmelConfig with the fields of the restatement's"""
    return pkg.LogmelConfig(**logmel_ref.config_fields(cfg))


def test_symbols_are_declared_and_exported(pkg):
    declared = pkg.declared_symbols(debug=False)
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/fmdemod.h"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.fmd_api_version() == 3
    for name in ("LogMel", "LogmelConfig", "LOGMEL_STATUS_DTYPE", "logmel_design", "logmel_max_frames", "logmel_default_config"):
        assert hasattr(pkg, name)
    assert pkg.LOGMEL_STATUS_DTYPE == logmel_ref.STATUS_DTYPE and pkg.LOGMEL_STATUS_DTYPE.itemsize == 32
    assert C.sizeof(pkg.LogmelConfig) == C.sizeof(logmel_ref.Config) == 72


@pytest.mark.parametrize("name", list(logmel_ref.GEOMETRIES))
def test_restatement_against_float64_by_the_apriori_bound(ref, name):
    """|mel32 - mel64| per band within logmel_ref.apriori_bound (derived from u = 2^-24, not measured) for noise at -20 dB, a 1 kHz tone
    at -12 dBFS and the tone over noise at -80 dB; powers, not logarithms: far from a tone the bands sit 100 dB down.  The worst ratio
    seen over the five geometries is 0.022."""
    g = logmel_ref.GEOMETRIES[name]
    cfg = logmel_ref.config(**dict(g, out_mode=0))
    fb = ref.design(cfg)[3]
    worst = 0.0
    for kind in SIGNALS:
        x = logmel_ref.signal(kind, cfg.fs, cfg.win + 6 * cfg.hop + 5)
        got = ref.run(cfg, x).astype(np.float64)
        want = logmel_ref.model_mel_power(cfg, x)
        bound = logmel_ref.apriori_bound(cfg, x, fb)
        assert got.shape == want.shape == (7, cfg.n_mels) and np.all(bound > 0.0)
        ratio = float(np.max(np.abs(got - want) / bound))
        print(f"{name} {kind}: worst |mel32 - mel64| / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        # the float32 filterbank against the float64 one: the model's own part of the difference is far inside the bound too
        assert np.abs(fb.astype(np.float64) - logmel_ref.model_filterbank(cfg)).max() <= 2.0 ** -24 * fb.max() * 1.01
    assert worst <= 1.0, worst


def test_log_rows_follow_the_powers(ref):
    """mode 1 is flog10 of the clamped mode-0 band, bit for bit"""
    g = logmel_ref.GEOMETRIES["8k"]
    x = logmel_ref.mixed_signal(8000, 64 + 16 * 20, ("tone", "silence", "noise"), 5, 1.0)
    p = ref.run(logmel_ref.config(**dict(g, out_mode=0)), x)
    l = ref.run(logmel_ref.config(**dict(g, out_mode=1)), x)
    assert np.array_equal(bits(l), bits(ref.flog10(np.maximum(p, np.float32(1e-10)))))
    assert (p == 0.0).any() and l.min() == -10.0                     # silence sits on the floor


@pytest.mark.parametrize("name", ["32k", "8k", "8k_htk"])
def test_framing_against_torch_stft(ref, name):
    """window, hop and bin conventions: float64 torch.stft, center=False, periodic Hann, cut to K bins == the model's frames; and the
    restatement's mel powers of a pure bin-centred tone peak in the band that holds it"""
    import torch
    cfg = logmel_ref.config(**dict(logmel_ref.GEOMETRIES[name], out_mode=0))
    x = logmel_ref.signal("noise", cfg.fs, cfg.win + 5 * cfg.hop + 3)
    m = torch.from_numpy(0.5 * (x[:, 0].astype(np.float64) + x[:, 1].astype(np.float64)))
    S = torch.stft(m, n_fft=cfg.win, hop_length=cfg.hop, win_length=cfg.win, window=torch.hann_window(cfg.win, periodic=True, dtype=torch.float64),
                   center=False, onesided=True, return_complex=True).numpy().T
    X, _ = logmel_ref.model_frames(cfg, x)
    K = ref.bins(cfg)
    assert X.shape == (6, K) and K == logmel_ref.model_bins(cfg)
    assert np.abs(S[:, :K] - X).max() <= 1e-12 * np.abs(X).max()
    got = ref.run(cfg, x).astype(np.float64)
    want = (np.abs(S[:, :K]) ** 2) @ logmel_ref.model_filterbank(cfg).T
    assert np.abs(got - want).max() <= 1e-4 * want.max()


def test_filterbank_known_answers(ref):
    assert ref.mel(1000.0, 0) == 15.0 and ref.mel(0.0, 0) == 0.0 and ref.mel(0.0, 1) == 0.0
    assert abs(ref.mel(1000.0, 1) - 1000.0) < 0.02
    for scale in (0, 1):
        for f in (0.0, 50.0, 999.0, 1000.0, 1001.0, 4000.0, 8000.0, 24000.0):
            assert abs(ref.mel_inv(ref.mel(f, scale), scale) - f) <= 1e-9 * max(f, 1.0), (scale, f)
            assert abs(ref.mel(f, scale) - float(logmel_ref.model_mel(f, scale))) <= 1e-9 * max(f, 1.0)
    for name, g in logmel_ref.GEOMETRIES.items():
        cfg = logmel_ref.config(**g)
        w, tc, ts, fb, K, empty = ref.design(cfg)
        assert empty == 0 and K == logmel_ref.model_bins(cfg), name
        assert w[0] == 0.0 and w[cfg.win // 2] == 1.0 and tc[0] == 1.0 and ts[0] == 0.0 and ts[cfg.win // 4] == 1.0
        width = (fb > 0).sum(axis=1)
        if cfg.mel_scale == 0:
            area = fb.astype(np.float64).sum(axis=1) * cfg.fs / cfg.win
            assert np.all(np.abs(area[width > 4] - 1.0) < 0.05), (name, area)
            assert (width > 4).any()
        else:
            assert fb.max() <= 1.0
    # a design made to have empty bands: 33 bins cannot feed 40 bands
    cfg = logmel_ref.config(fs=8000, win=64, hop=16, n_mels=40)
    fb, empty = ref.design(cfg)[3], ref.design(cfg)[5]
    assert empty == int((fb.max(axis=1) == 0.0).sum()) and empty > 0
    assert empty == int((logmel_ref.model_filterbank(cfg).astype(np.float32).max(axis=1) == 0.0).sum())


def test_flog10_within_8_ulp(ref):
    """the condition of the contract: no more than 8 fp32 ulp from float64 log10, on every 1021st finite float >= FLT_MIN and on every
    float in [0.5, 2); the exhaustive figure (tools/logmel_flog10_sweep.cpp) is in DESIGN.md §6n"""
    worst, at, count = ref.flog10_sweep(0x00800000, 0x7F7FFFFF, 1021)
    print(f"strided: worst {worst:.4f} ulp at 0x{at:08x} over {count} floats")
    assert count == (0x7F7FFFFF - 0x00800000) // 1021 + 1 and worst <= 8.0
    worst, at, count = ref.flog10_sweep(0x3F000000, 0x3FFFFFFF, 1)
    print(f"[0.5, 2): worst {worst:.4f} ulp at 0x{at:08x} over {count} floats")
    assert count == 1 << 24 and worst <= 8.0
    tiny, big = np.float32(logmel_ref.FLT_MIN), np.float32(logmel_ref.FLT_MAX)
    y = ref.flog10(np.array([tiny, big, 1.0, 1e-10, 10.0, 100.0, 0.1], np.float32))
    assert y[2] == 0.0
    for got, x in zip(y, (tiny, big, 1.0, np.float32(1e-10), 10.0, 100.0, np.float32(0.1))):
        want = math.log10(float(x))
        assert abs(float(got) - want) <= 8 * np.spacing(np.float32(abs(want))) , (x, got, want)
    sp = ref.flog10(np.array([np.inf, np.nan], np.float32))
    assert sp[0] == np.inf and np.isnan(sp[1])
    # the clamp: a band at or under the floor reads the floor, a NaN band stays NaN, +inf stays
    assert ref.clamp(0.0, 1e-10) == np.float32(1e-10) and ref.clamp(np.float32(1e-10), 1e-10) == np.float32(1e-10) and ref.clamp(2.0, 1e-10) == 2.0
    assert math.isnan(ref.clamp(math.nan, 1e-10)) and ref.clamp(math.inf, 1e-10) == math.inf
    assert ref.out(0.0, 1, 1e-10) == -10.0 and ref.out(0.0, 0, 1e-10) == 0.0 and ref.out(math.inf, 1, 1e-10) == math.inf
    for mode in (0, 1):                                           # any NaN leaves as 0x7fc00000
        v = np.array([ref.out(float(np.array([0xFFC12345], np.uint32).view(np.float32)[0]), mode, 1e-10)], np.float32)
        assert bits(v)[0] == 0x7FC00000


def test_restatement_split_invariance(ref):
    """one call, a call per hop and ragged calls give the same rows and records; T(f) at its edges; fmd_logmel_max_frames reached and
    never exceeded; hop = win; a reset mid-window"""
    for g in (dict(fs=8000, win=64, hop=16, n_mels=8), dict(fs=8000, win=64, hop=24, n_mels=8), dict(fs=8000, win=64, hop=64, n_mels=8),
              dict(fs=8000, win=80, hop=16, n_mels=8)):
        cfg = logmel_ref.config(**g)
        N, hop = cfg.win, cfg.hop
        n = N + hop * 12 + 7
        x = logmel_ref.mixed_signal(cfg.fs, n, ("noise", "tone", "tone_noise", "silence"), 11, 0.7)
        whole = ref.channel(cfg)
        rows = whole.process(x)
        assert rows.shape[0] == ref.T(n, N, hop) == (n - N) // hop + 1
        for cuts in (list(range(hop, n, hop)), [1, 8, 23, 39, 56, 119, 183, 248], list(range(1, n, 1)) if hop == 16 and N == 64 else [N - 1, N, N + 1]):
            ch, got, at = ref.channel(cfg), [], 0
            for c in cuts + [n]:
                before = int(ch.status()["frames"][0])
                r = ch.process(x[at:c])
                assert r.shape[0] == ref.T(before + c - at, N, hop) - ref.T(before, N, hop) <= ref.max_frames(hop, c - at)
                got.append(r)
                at = c
            assert np.array_equal(bits(np.concatenate(got)), bits(rows)), (g, cuts[:4])
            assert ch.status().tobytes() == whole.status().tobytes()
        st = whole.status()[0]
        assert st["frames"] == n and st["spectra"] == rows.shape[0] and st["fill"] == n - rows.shape[0] * hop and st["nonfinite"] == 0
        for f, t in ((0, 0), (N - 1, 0), (N, 1), (N + hop - 1, 1), (N + hop, 2)):
            assert ref.T(f, N, hop) == t
        # the most frames of a call of n: a station one sample short of a window completes (n + hop - 1) / hop of them
        ch = ref.channel(cfg)
        ch.process(x[:N - 1])
        for k in (1, hop, hop + 1, 3 * hop):
            before = int(ch.status()["frames"][0])
            assert ch.process(x[before:before + k]).shape[0] == ref.max_frames(hop, k) or (before - (N - 1)) % hop != 0
        # reset mid-window: as a fresh station
        ch = ref.channel(cfg)
        ch.process(x[:N + 5])
        ch.reset()
        assert ch.status().tobytes() == ref.channel(cfg).status().tobytes()
        assert np.array_equal(bits(ch.process(x)), bits(rows))
    assert ref.T((1 << 40) + 64, 64, 16) == (1 << 36) + 1


def test_nonfinite_samples_make_nonfinite_frames(ref):
    cfg = logmel_ref.config(fs=8000, win=64, hop=16, n_mels=8)
    x = logmel_ref.signal("noise", 8000, 64 + 16 * 9)
    x[100, 0] = np.inf
    x[170, 1] = np.nan
    ch = ref.channel(cfg)
    rows = ch.process(x)
    bad = ~np.isfinite(rows).all(axis=1)
    want = np.array([t * 16 <= 100 < t * 16 + 64 or t * 16 <= 170 < t * 16 + 64 for t in range(10)])
    assert np.array_equal(bad, want) and ch.status()["nonfinite"][0] == want.sum()
    assert np.all(bits(rows[bad])[np.isnan(rows[bad])] == 0x7FC00000)


def test_library_host_functions_equal_the_restatement(pkg, ref):
    """the library's design, bins, default configuration, max_frames and flog10 == the restatement's, bit for bit; every argument bound
    from both sides"""
    for name, g in logmel_ref.GEOMETRIES.items():
        cfg = logmel_ref.config(**g)
        got, want = pkg.logmel_tables(_lib_config(pkg, cfg)), ref.design(cfg)
        for a, b in zip(got[:4], want[:4]):
            assert np.array_equal(bits(a), bits(b)), name
        assert got[4:] == want[4:]
        w, fb, K, empty = pkg.logmel_design(_lib_config(pkg, cfg))
        assert np.array_equal(bits(w), bits(want[0])) and np.array_equal(bits(fb), bits(want[3])) and (K, empty) == want[4:]
    for fs, win, hop in ((8000, 208, 80), (16000, 400, 160), (22050, 560, 220), (32000, 800, 320), (44100, 1104, 441), (48000, 1200, 480)):
        got, want = pkg.logmel_default_config(fs), ref.default_config(fs)
        assert logmel_ref.config_fields(got) == logmel_ref.config_fields(want)
        assert (got.win, got.hop, got.n_mels, got.f_min_hz, got.f_max_hz, got.mel_scale, got.out_mode) == (win, hop, 80, 0.0, min(8000.0, fs / 2), 0, 1)
        assert np.float32(got.log_floor) == np.float32(1e-10) and ref.check(want) == 0
    for fs in (7999, 48001):
        assert ref.default_config(fs) is None
        with pytest.raises(pkg.FmdError):
            pkg.logmel_default_config(fs)
    base = dict(fs=8000, win=64, hop=16, n_mels=8, f_min_hz=0.0, f_max_hz=3000.0)
    edges = [("fs", 8000, 7999), ("fs", 48000, 48001), ("win", 64, 48), ("win", 2048, 2064), ("win", 80, 72), ("hop", 16, 15), ("hop", 64, 65), ("n_mels", 1, 0),
             ("n_mels", 128, 129), ("f_min_hz", 0.0, -1e-9), ("f_min_hz", 2999.0, 3000.0), ("f_max_hz", 4000.0, 4000.001), ("mel_scale", 1, 2), ("mel_scale", 0, -1),
             ("out_mode", 1, 2), ("out_mode", 0, -1), ("log_floor", logmel_ref.FLT_MIN, logmel_ref.FLT_MIN / 2), ("log_floor", logmel_ref.FLT_MAX, math.inf),
             ("log_floor", 1.0, math.nan), ("max_input_frames", 1, 0), ("max_input_frames", 1 << 30, (1 << 30) + 1), ("n_channels", 1, 0)]
    L = pkg.load_library()
    for field, good, bad in edges:
        for v, ok in ((good, True), (bad, False)):
            cfg = logmel_ref.config(**{**base, field: v})
            assert (ref.check(cfg) == 0) == ok, (field, v)
            rc = L.fmd_logmel_bins(C.byref(_lib_config(pkg, cfg)))
            assert (rc == ref.bins(cfg)) if ok else (rc == -1 and L.fmd_logmel_last_error(None)), (field, v)
    for hop, n in ((16, 0), (16, 1), (16, 16), (16, 17), (320, 2048), (2048, 1 << 40), (24, 1000)):
        assert pkg.logmel_max_frames(hop, n) == ref.max_frames(hop, n) == (n + hop - 1) // hop
    for hop, n in ((15, 1), (2049, 1), (16, -1), (16, (1 << 40) + 1)):
        assert ref.max_frames(hop, n) == -1
        with pytest.raises(pkg.FmdError):
            pkg.logmel_max_frames(hop, n)
    x = np.concatenate([np.array([logmel_ref.FLT_MIN, logmel_ref.FLT_MAX, 1.0, 1e-10, np.inf], np.float32),
                        np.random.default_rng(3).uniform(0.0, 1.0, 2000).astype(np.float32) ** 8 * 1e6 + np.float32(logmel_ref.FLT_MIN)])
    assert np.array_equal(bits(pkg.logmel_flog10(x)), bits(ref.flog10(x)))


def _design_args(sets):
    return [repr(float(v)) if i in (4, 5) else str(v) for s in sets for i, v in enumerate(s)]


DESIGN_SETS = ((32000, 800, 320, 80, 0.0, 8000.0, 0), (8000, 64, 16, 8, 0.0, 4000.0, 0), (8000, 64, 24, 8, 100.0, 3000.0, 1), (44100, 1104, 441, 80, 0.0, 8000.0, 0),
               (48000, 2048, 16, 128, 20.0, 24000.0, 1))


def _check_design_program(ref, exe, tmp_path):
    r = subprocess.run([str(exe), str(tmp_path)] + _design_args(DESIGN_SETS), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok"
    for i, s in enumerate(DESIGN_SETS):
        cfg = logmel_ref.config(fs=s[0], win=s[1], hop=s[2], n_mels=s[3], f_min_hz=s[4], f_max_hz=s[5], mel_scale=s[6])
        w, tc, ts, fb, K, empty = ref.design(cfg)
        assert lines[i].split() == [str(K), str(empty)], s
        got = np.fromfile(tmp_path / f"logmel_{i}.f32", np.float32)
        assert np.array_equal(bits(got), bits(np.concatenate([w, tc, ts, fb.reshape(-1)]))), s
    for line, fs in zip(lines[len(DESIGN_SETS):], (8000, 16000, 22050, 32000, 44100, 48000)):
        d = ref.default_config(fs)
        assert line.split() == ["default", str(fs), str(d.win), str(d.hop), str(ref.bins(d)), str(ref.design(d)[5])]


def test_host_unit_under_sanitizers(ref, tmp_path):
    """fmd_logmel_design.cpp and tests/cpp/logmel_design_main.cpp, built with -fsanitize=address,undefined and run as a stand-alone
    program: clean, with exact-size arrays at the smallest and largest valid designs and at invalid ones; the tables it writes are the
    restatement's, bit for bit"""
    exe = tmp_path / "logmel_design_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{csrc}", str(csrc / "fmd_logmel_design.cpp"),
                    str(ROOT / "tests" / "cpp" / "logmel_design_main.cpp"), "-o", str(exe)], check=True)
    _check_design_program(ref, exe, tmp_path)


def test_library_design_equals_the_restatement(pkg, ref, tmp_path):
    """the same program linked with libfmdemod.so itself, so that the tables are those of the library as it is built (its compiler and
    flags, not this test's)"""
    exe = tmp_path / "logmel_design_lib"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{csrc}", str(ROOT / "tests" / "cpp" / "logmel_design_main.cpp"),
                    f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    _check_design_program(ref, exe, tmp_path)


def test_flog10_header_equals_the_restatement(ref, tmp_path):
    """fmd_logmel_math.h (what the kernel compiles) built for the host == the restatement's flog10 on a strided sweep, bit for bit"""
    src = tmp_path / "f.cpp"
    src.write_text(r'''
#include "fmd_logmel_math.h"
#include <stdio.h>
int main() {
    for (unsigned long long b = 0x00800000ull; b <= 0x7f800000ull; b += 4099) { const float y = fmd::flog10(fmd::lm_bits_f32((uint32_t)b)); fwrite(&y, 4, 1, stdout); }
    return 0;
}''')
    exe = tmp_path / "f"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'fm-radio_amd' / 'csrc'}", str(src), "-o", str(exe)], check=True)
    got = np.frombuffer(subprocess.run([str(exe)], check=True, capture_output=True).stdout, np.float32)
    x = np.arange(0x00800000, 0x7F800001, 4099, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert got.size == x.size and np.array_equal(bits(got), bits(ref.flog10(x)))


def test_lds_layout_fits(pkg, tmp_path):
    """the kernel's LDS image stays within 64 KB with at least one row at every corner of the configuration space, and takes 16 rows at
    the default geometries"""
    src = tmp_path / "l.cpp"
    src.write_text(r'''
#include "fmd_logmel_design.h"
#include <stdio.h>
int main() {
    for (int win = 64; win <= 2048; win += 16)
        for (int hop : {16, win / 2, win})
            for (double fmax : {100.0, 4000.0}) {
                fmd_logmel_config c; fmd_logmel_default_config(8000, &c); c.win = win; c.hop = hop < 16 ? 16 : hop; c.f_max_hz = fmax; c.n_mels = 128;
                std::string e; if (fmd::logmel_check(&c, &e) != FMD_OK) return 2;
                const fmd::LogmelLayout L = fmd::logmel_layout(&c);
                if (L.rows < 1 || L.rows > 16 || L.total * 4 > fmd::kLogmelLdsBytes || L.span != (L.rows - 1) * c.hop + win || L.Kp % 16 || L.Kp < L.K || L.Mp != 128) return 3;
                if (L.off_tab != win || L.off_m != 3 * win || L.off_p != L.off_m + L.span || L.off_nf != L.off_p + L.rows * L.Kp || L.total != L.off_nf + 16) return 4;
            }
    for (int fs : {8000, 16000, 22050, 32000, 44100, 48000}) {
        fmd_logmel_config c; fmd_logmel_default_config(fs, &c);
        printf("%d %d\n", fs, fmd::logmel_layout(&c).rows);
    }
    return 0;
}''')
    exe = tmp_path / "l"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O1", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{csrc}", str(src), str(csrc / "fmd_logmel_design.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.returncode
    rows = dict(tuple(map(int, l.split())) for l in r.stdout.strip().split("\n"))
    assert rows[32000] == 16 and rows[16000] == 16 and rows[8000] == 16, rows
