"""Batched audio resampler, the parts that need no GPU:
  * the C restatement of the reference's Resample (tests/cpp/resample_ref.c) against the reference's own outputs
    (tests/golden/resample_ref.npz, made once from the reference built with its own flags; DESIGN.md "Audio resampler"),
  * the polyphase prototype (fmd_resampler_design) against its specification,
  * the C restatement of the polyphase method (tests/cpp/resample_poly_ref.c) against float64 under the fp32 chain's a-priori bound, its
    split invariance, resets and pcm16, and the (L, M, T, tile) of every case test_gpu_resample_poly.py holds the GPU to it at,
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


@pytest.fixture(scope="module")
def PolyRef(tmp_path_factory):
    return resample_ref.build_poly(tmp_path_factory.mktemp("resample_poly_ref"))


def _case_id(case):
    return f"{case[0]}-{case[1]}-T{case[2]}"


def _poly_case(pkg, case):
    fs_in, fs_out, tpp = case
    taps, L, M = pkg.resampler_design(fs_in, fs_out, taps_per_phase=tpp)
    return taps, L, M


@pytest.mark.parametrize("case", sorted(resample_ref.POLY_CASES), ids=_case_id)
def test_polyphase_cases_have_the_ratio_taps_and_tile_they_are_meant_to(pkg, case):
    """(L, M, T, tile) of every polyphase case, against the literals: T from fmd_resampler_design, tile from the halving rule.  A case meant
    for tile 128 (32000 -> 4000) or tile 32 (32000 -> 1000 with 256 taps per phase) cannot silently become a tile-256 case."""
    taps, L, M = _poly_case(pkg, case)
    assert (L, M, taps.shape[0], resample_ref.poly_tile(L, M, taps.shape[0])) == resample_ref.POLY_CASES[case]
    tiles = {c[:2] + (c[2],): v[3] for c, v in resample_ref.POLY_CASES.items()}
    assert tiles[(32000, 4000, 0)] == 128 and tiles[(32000, 1000, 256)] == 32
    assert all(v == 256 for c, v in tiles.items() if c not in {(32000, 4000, 0), (32000, 1000, 256)})
    # the three calls the GPU test feeds: two full tiles and a ragged third, one tile (or the next count an up-sampler can emit), under 64
    tile, pos, counts = resample_ref.POLY_CASES[case][3], 0, []
    for k in resample_ref.poly_three_calls(L, M, tile):
        counts.append(resample_ref.poly_count(pos, k, L, M))
        pos += k
    assert 2 * tile + 17 <= counts[0] < 3 * tile and 37 <= counts[2] < 64
    assert counts[1] == (258 if case[1] == 192000 else tile), counts


@pytest.mark.parametrize("case", sorted(resample_ref.POLY_CASES), ids=_case_id)
def test_polyphase_restatement_within_the_chain_bound_of_float64(pkg, PolyRef, case):
    """The C restatement against polyphase_f64 with the same fp32 taps: every value within gamma_T sum_t |h_t| |x_t|, gamma_T = T u / (1 - T u),
    u = 2^-24: the a-priori bound of a T-term fp32 FMA chain started at 0 (each fmaf rounds once; nothing here underflows), computed per
    output in float64.  No measured constant: the worst ratio is printed, not asserted (DESIGN.md "Audio resampler" lists it per case)."""
    taps, L, M = _poly_case(pkg, case)
    T = taps.shape[0]
    n = sum(resample_ref.poly_three_calls(L, M, resample_ref.POLY_CASES[case][3]))
    x = resample_ref.noise_and_tone(2, n, seed=3, fs_in=case[0])
    got = PolyRef(2, L, M, taps).process(x)
    n1 = -(-n * L // M)
    assert got.shape == (2, n1, 2)
    u = 2.0 ** -24
    gamma = T * u / (1.0 - T * u)
    worst = 0.0
    for c in range(2):
        e = resample_ref.polyphase_f64(x[c], taps, L, M, 0, n1)
        bound = gamma * resample_ref.polyphase_f64(np.abs(x[c]), np.abs(taps), L, M, 0, n1)
        err = np.abs(got[c].astype(np.float64) - e)
        assert np.all(err <= bound), (c, int(np.argmax(err - bound)), float(np.max(err - bound)))
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    print(f"polyphase restatement {case}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("fs_out", [44100, 22050, 8000, 4000])
def test_polyphase_restatement_is_split_invariant(pkg, PolyRef, fs_out):
    """One call against 3 T frames and then 1, 1, 1, 0, 2, T - 2, T - 1, T, T + 1, 1, 5 T + 3, 1, 1 (n = 0 and calls that emit nothing
    included): the same bits, and each call emits ceil((pos + k) L / M) - ceil(pos L / M) frames."""
    taps, L, M = pkg.resampler_design(32000, fs_out)
    T = taps.shape[0]
    splits = [3 * T] + resample_ref.poly_call_shapes(T)
    x = resample_ref.noise_and_tone(3, sum(splits), seed=4)
    whole = PolyRef(3, L, M, taps).process(x)
    assert whole.shape[1] == -(-sum(splits) * L // M)
    r = PolyRef(3, L, M, taps)
    parts, pos, counts = [], 0, []
    for k in splits:
        want = resample_ref.poly_count(pos, k, L, M)
        assert r.output_frames(k) == want
        y = r.process(x[:, pos:pos + k])
        assert y.shape[1] == want
        counts.append(want)
        parts.append(y)
        pos += k
        assert r.counters() == (pos, -(-pos * L // M))
    assert bits_equal(np.concatenate(parts, axis=1), whole)
    assert splits[4] == 0 and counts[4] == 0
    if fs_out in (8000, 4000):
        assert any(k > 0 and n == 0 for k, n in zip(splits, counts)), counts


def test_polyphase_restatement_resets_and_pcm16(pkg, PolyRef):
    """reset(c) zeroes channel c's past and keeps the counters; reset(-1) starts over.  pcm16 is the low 16 bits of (int32)(y * 31128.65f),
    modular, and NaN, +-inf and |t| >= 2^31 are reported as unspecified."""
    taps, L, M = pkg.resampler_design(32000, 8000)
    T = taps.shape[0]
    x = resample_ref.noise_and_tone(3, 4 * T + 7, seed=5)
    a, b = PolyRef(3, L, M, taps), PolyRef(3, L, M, taps)
    k = 3 * T + 7
    first = a.process(x[:, :k])
    b.process(x[:, :k])
    b.reset(1)
    assert b.counters() == a.counters()
    ya, yb = a.process(x[:, k:]), b.process(x[:, k:])
    assert bits_equal(ya[0], yb[0]) and bits_equal(ya[2], yb[2]) and not bits_equal(ya[1], yb[1])
    # channel 1 after its reset: the stream with everything before frame k zero
    z = x.copy()
    z[1, :k] = 0.0
    c = PolyRef(3, L, M, taps)
    c.process(z[:, :k])
    assert bits_equal(c.process(z[:, k:])[1], yb[1])
    b.reset(-1)
    assert b.counters() == (0, 0)
    assert bits_equal(b.process(x[:, :k]), first)
    y = np.array([0.0, 0.5, -0.5, 1.0, 1.06, -1.06, 2.2, 68000.0, -68000.0, 68900.0, np.nan, np.inf, -np.inf, 1e38], np.float32)
    p, un = PolyRef.pcm16(y)
    t = (y[:10] * (np.float32(32767.0) * np.float32(0.95))).astype(np.float64)
    want = ((np.trunc(t).astype(np.int64) + 32768) % 65536 - 32768).astype(np.int16)
    assert np.array_equal(p[:10], want) and not un[:10].any() and un[10:].all()
    assert want[4] < 0 < want[5] and 2.0 ** 31 - 2.0 ** 24 < abs(t[9]) < 2.0 ** 31      # wraps, right up to the int32 edge


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
