"""Batched audio resampler, the parts that need no GPU:
  * the C restatement of the reference's Resample (tests/cpp/resample_ref.c) against the reference's own outputs
    (tests/golden/resample_ref.npz, made once from the reference built with its own flags; DESIGN.md "Audio resampler"),
  * the polyphase prototype (fmd_resampler_design) against its specification,
  * the player adaptor header and its driver compile against the C ABI alone.
"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import resample_ref
from conftest import GOLDEN, bits_equal, describe_diff

ROOT = Path(__file__).resolve().parent.parent
RATES = {48000: (3, 2), 44100: (441, 320), 22050: (441, 640), 16000: (1, 2), 8000: (1, 4)}


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    return p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return resample_ref.build(tmp_path_factory.mktemp("resample_ref"))


def test_restatement_is_bit_identical_to_the_reference_fixture(ref):
    g = np.load(GOLDEN / "resample_ref.npz")
    cases = [str(c) for c in g["cases"]]
    rejected = {str(c) for c in g["rejected"]}
    assert len(cases) == 8 and rejected == {"n16384_fs48000"}
    for key in cases:
        N, fs = (int(v[1:] if v[0] == "n" else v[2:]) for v in key.split("_"))
        if key in rejected:
            x = np.zeros((N, 2), np.float32)            # the index chain does not depend on the samples
            assert ref(x, fs) is None, key
            continue
        y = ref(g[key + "_in"], fs)
        assert y is not None and bits_equal(y, g[key + "_out"]), (key, describe_diff(y, g[key + "_out"]))


def test_restatement_passes_equal_rates_through(ref):
    x = np.random.default_rng(1).standard_normal((777, 2)).astype(np.float32)
    assert bits_equal(ref(x, 32000), x)


@pytest.mark.parametrize("fs_out", sorted(RATES))
def test_polyphase_design(pkg, fs_out):
    taps, L, M = pkg.resampler_design(32000, fs_out)
    assert (L, M) == RATES[fs_out]
    T = taps.shape[0]
    assert taps.shape == (32 * -(-M // L), L) and taps.dtype == np.float32
    # every phase passes DC with gain 1
    assert np.max(np.abs(taps.astype(np.float64).sum(0) - 1.0)) < 1e-6
    # the prototype h[p + t L] at the up-sampled rate L * 32 kHz: gain L in the passband, >= 60 dB down from min(fs_in, fs_out) / 2
    h = taps.reshape(-1).astype(np.float64)
    nfft = 1 << 20
    H = np.abs(np.fft.rfft(h, nfft)) / L
    f = np.arange(H.size) / nfft * (L * 32000.0)
    f_stop = min(32000, fs_out) / 2
    assert 20 * np.log10(H[f >= f_stop].max()) <= -60.0
    # passband: flat within 0.1 dB up to 60 % of the stopband edge (the default T: the transition takes the rest)
    pb = H[f <= 0.6 * f_stop]
    assert np.max(np.abs(20 * np.log10(pb))) < 0.1


def test_design_rejects_what_it_cannot_build(pkg):
    with pytest.raises(pkg.FmdError):
        pkg.resampler_design(32000, 0)
    with pytest.raises(pkg.FmdError):
        pkg.resampler_design(32000, 48000, taps_per_phase=6)


def test_player_adaptor_compiles_against_the_c_abi_alone(tmp_path):
    exe = tmp_path / "resample_player_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}",
                    str(ROOT / "tests" / "cpp" / "resample_player_main.cpp"), f"-L{ROOT / 'fm-radio_amd' / 'csrc'}", "-lfmdemod", "-o", str(exe)],
                   check=True)
    assert exe.exists()
