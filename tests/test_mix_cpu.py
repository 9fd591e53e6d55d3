"""Batched audio mixer, the parts that need no GPU:
  * the C restatement of the reference's UpdateMixer (tests/cpp/mix_ref.c) against the reference's own outputs (tests/golden/mix_ref.npz,
    recorded once from the reference's AudioMixer and RingBuffer built with its own flags),
  * the fixture pins the reference's log10f: a float64 log10 rounded to float does not reproduce it where log10f is not correctly rounded,
  * the mixer adaptor header and its driver compile against the C ABI alone.
"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mix_ref
from conftest import GOLDEN, bits_equal, describe_diff

ROOT = Path(__file__).resolve().parent.parent
CASES = {"one_g1", "one_clip", "one_clip_neg", "two", "three", "four", "n23", "n25", "n64_a40", "n3_none", "special", "special_g3",
         "gain_denormal", "gain_denormal_neg", "scale_denormal"}


@pytest.fixture(scope="module")
def mix(tmp_path_factory):
    return mix_ref.build(tmp_path_factory.mktemp("mix_ref"))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "mix_ref.npz")


def test_fixture_holds_the_cases(golden):
    assert {str(c) for c in golden["cases"]} == CASES
    assert golden["n64_a40_active"].sum() == 40 and golden["n3_none_active"].sum() == 0
    sp = golden["special_in"]
    assert np.isnan(sp).any() and np.isinf(sp).any() and ((sp != 0) & (np.abs(sp) < np.finfo(np.float32).tiny)).any()
    assert (np.signbit(golden["special_out"]) & (golden["special_out"] == 0)).any()      # flushed results keep their sign


def test_restatement_is_bit_identical_to_the_reference_fixture(mix, golden):
    for key in sorted(CASES):
        x, act, gain, want = mix_ref.fixture_case(golden, key)
        got = mix(x, np.arange(x.shape[0]), act, gain)
        assert bits_equal(got, want), (key, describe_diff(got, want))


def test_fixture_pins_log10f(mix, golden):
    """At 23 and 25 sources glibc's log10f is not correctly rounded: the same restatement with a float64 log10 gives other bits there and
    the same bits where the two logarithms agree."""
    for key in ("n23", "n25"):
        x, act, gain, want = mix_ref.fixture_case(golden, key)
        assert not bits_equal(mix(x, np.arange(x.shape[0]), act, gain, f64_log=True), want), key
        k = int(act.sum())
        assert mix.lib.mix_ref_scale(gain, k, 0) != mix.lib.mix_ref_scale(gain, k, 1)
    for key in ("two", "four"):
        x, act, gain, want = mix_ref.fixture_case(golden, key)
        assert bits_equal(mix(x, np.arange(x.shape[0]), act, gain, f64_log=True), want), key


def test_restatement_rules(mix):
    f = np.float32
    x = np.zeros((3, 6, 2), f)
    x[0, :, 0] = [np.nan, -np.nan, np.inf, -np.inf, 1e-40, 5.0]
    y = mix(x, [0, 1, 2], None, 1.0)
    assert list(y[:4, 0]) == [1.0, 1.0, 1.0, -1.0] and y[4, 0] == 0.0 and y[5, 0] == 1.0
    # no delivering source: every output is +0
    z = mix(x, [0, 1, 2], np.zeros(3, np.uint8), 1.0)
    assert not np.signbit(z).any() and not z.any()
    # an empty bus
    assert not mix(x, [], None, 1.0).any()


def test_mixer_adaptor_compiles_against_the_c_abi_alone(tmp_path):
    exe = tmp_path / "mixer_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}",
                    str(ROOT / "tests" / "cpp" / "mixer_main.cpp"), f"-L{ROOT / 'fm-radio_amd' / 'csrc'}", "-lfmdemod", "-o", str(exe)],
                   check=True)
    assert exe.exists()
