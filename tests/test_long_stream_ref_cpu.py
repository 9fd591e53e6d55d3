"""The helpers of the long-stream GPU tests (tests/long_stream_ref.py), checked without a GPU: the restatement at a start index against
test_channelizer.ref_channelize, the library's phase increment at dyadic offsets, the period conditions of every case the GPU file uses,
and the expected totals of the IQ corrector."""
from fractions import Fraction

import numpy as np
import pytest

import long_stream_ref as LS
from test_channelizer import ref_channelize


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    return p


# small rate pairs of the kinds the channeliser meets: L = 16, L = 1, L = 8 (fs_in, fs_out, taps per phase)
SMALL = [(1_000_000.0, 256_000.0, 24), (2_048_000.0, 256_000.0, 32), (2_400_000.0, 256_000.0, 16)]


@pytest.mark.parametrize("fs_in,fs_out,tpp", SMALL)
def test_start_index_zero_is_ref_channelize(pkg, fs_in, fs_out, tpp):
    rng = np.random.default_rng(1)
    taps, L, M = pkg.chan_design(fs_in, fs_out, tpp)
    P = M * 7 * (16 // np.gcd(16, L))
    x = rng.standard_normal(P) + 1j * rng.standard_normal(P)
    for f in (0.0, -0.31 * fs_in + 1234.5, fs_in * 3 / 32):
        want = ref_channelize(x, f, taps, L, M, fs_in=fs_in)
        got = LS.ref_channelize_at(x, 0, want.size, f, fs_in, taps, L, M)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("fs_in,fs_out,tpp", SMALL)
def test_start_index_k_periods_is_ref_channelize_over_k_plus_one(pkg, fs_in, fs_out, tpp):
    rng = np.random.default_rng(2)
    taps, L, M = pkg.chan_design(fs_in, fs_out, tpp)
    P = M * 80
    n_call = P * L // M
    x = rng.standard_normal(P) + 1j * rng.standard_normal(P)
    for k, f in ((1, 0.27 * fs_in + 1234.5), (3, -fs_in * 5 / 64), (6, -0.449 * fs_in)):
        whole = ref_channelize(np.tile(x, k + 1), f, taps, L, M, fs_in=fs_in)
        got = LS.ref_channelize_at(x, k * P, n_call, f, fs_in, taps, L, M)
        want = whole[k * n_call:]
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
        # a start inside a period, at a whole output
        o = (n_call // 3) // L * L
        got = LS.ref_channelize_at(x, k * P + o * M // L, 20, f, fs_in, taps, L, M)
        assert np.abs(got - want[o:o + 20]).max() <= 1e-10 * np.abs(want).max()


def test_outputs_at_a_crossing_are_those_of_the_whole_stream(pkg):
    """ChanCase.window / chan_outputs_at, as the GPU tests use them, on a stream short enough to restate whole"""
    fs_in, tpp = 1_000_000.0, 24
    rng = np.random.default_rng(3)
    taps, L, M = pkg.chan_design(fs_in, 256_000.0, tpp)
    assert (L, M) == (32, 125)
    n_c = 2 * 48_000 + 12_345
    case = LS.ChanCase(fs_in, L, M, [(3, 5), (-5, 6)], [0.33 * fs_in + 1234.5], P=48_000, crossings=(n_c,), wraps=())
    assert case.n_out == 3 * 4096 and case.n_calls == 5
    x = rng.standard_normal(case.P) + 1j * rng.standard_normal(case.P)
    call, o_lo, n_call, cnt = case.window(n_c)
    assert (call, n_call, cnt) == (2, 2 * 48_000, 2 * LS.HALF)
    o_abs = call * case.n_out + o_lo
    newest = (np.arange(o_abs, o_abs + cnt) * M) // L
    assert newest[0] < n_c - tpp and newest[LS.HALF - 1] < n_c <= newest[LS.HALF] and newest[-1] - tpp > n_c
    for k, f in enumerate(case.centers):
        whole = ref_channelize(np.tile(x, 4), f, taps, L, M, fs_in=fs_in)
        got = LS.chan_outputs_at(case, x, n_c, taps, k)
        assert np.abs(got - whole[o_abs:o_abs + cnt]).max() <= 1e-10 * np.abs(whole).max()


def test_exact_phase_at_a_large_index():
    """one tap, x = 1: the output is the phasor itself.  At n = 2^32 + 12345 it is the exactly reduced phase, which the float64 product
    f / fs n misses by more than 1e-7 rad"""
    fs_in, f, L, M = 20_480_000.0, 0.33 * 20_480_000 + 1234.5, 1, 80
    taps = np.ones((1, 1), np.float32)
    n0 = ((LS.TWO32 + 12345) // M) * M
    y = LS.ref_channelize_at(np.ones(M * 4), n0, 1, f, fs_in, taps, L, M)[0]
    fr = Fraction(f) / Fraction(fs_in)
    exact = float((n0 * fr) % 1)
    assert abs(np.angle(y * np.exp(2j * np.pi * exact))) < 1e-12
    naive = (f / fs_in * n0) % 1.0
    assert abs(naive - exact) > 1e-8


def test_dyadic_offsets_have_exact_increments_that_vanish_over_a_period():
    for fs_in in (10e6, 2.4e6, 20.48e6, 20e6, 25e6):
        for a, k in ((3, 5), (-5, 6), (1, 12), (-2047, 12)):
            inc = LS.library_phase_inc(fs_in * a / (1 << k), fs_in)
            assert inc == (a % (1 << k)) << (64 - k)              # exact: no rounding in f / fs_in, none in the increment
            assert (inc * (1 << k) * 3) % (1 << 64) == 0
    assert LS.library_phase_inc(1234.5, 10e6) % 2 == 0            # the library's increments are even
    assert (LS.library_phase_inc(1234.5, 10e6) * LS.chan_period(16, 625)) % (1 << 64) != 0    # an arbitrary offset does not repeat


def test_period_conditions_hold_for_every_gpu_case():
    import test_gpu_long_streams as G
    assert len(G.CHAN_CASES) == 12
    for name, case, fmt in G.CHAN_CASES:
        c = case()                                               # ChanCase asserts its conditions
        assert c.n_calls * c.P > LS.TWO32 + 2 * c.P, name
        assert c.n_dyadic == 2 and len(c.centers) == 3 and c.dyadic[0] > 0 > c.dyadic[1], name
    fmts = [fmt for _, _, fmt in G.CHAN_CASES]
    assert fmts.count("cf32") == 6 and all(fmts.count(f) >= 2 for f in ("u8", "s8", "s16"))
    c = G.output_index_case()
    assert c.crossings == (LS.TWO31 * 75 // 8, LS.TWO32 * 75 // 8) and c.n_calls * c.n_out > LS.TWO32 + 2 * c.n_out
    assert [c.crossing(n_c)[0] * c.n_out + c.crossing(n_c)[1] for n_c in c.crossings] == [LS.TWO31, LS.TWO32]
    # the example of 20.48 MSa/s
    c = LS.ChanCase(20.48e6, 1, 80, [(3, 5), (-5, 6)], [1234.5])
    assert (c.P, c.n_out, LS.TWO32 % c.P) == (1_966_080, 24_576, 1_048_576)
    # what the conditions refuse: a period that divides 2^32, and one whose calls are not whole tiles
    with pytest.raises(AssertionError):
        LS.ChanCase(2.048e6, 1, 8, [(3, 5)], [], P=8 * 4096 * 64, crossings=())
    with pytest.raises(AssertionError):
        LS.ChanCase(20.48e6, 1, 80, [(3, 5)], [], P=80 * 3 * 1000, crossings=())
    # the resampler, the IQ corrector and the scanner
    for L, M in G.RESAMPLE_RATIOS.values():
        assert (G.RS_P * L) % M == 0 and (G.RS_P * L // M) % 256 == 0
    for P in (G.RS_P, G.IQ_P, G.SCAN_P):
        assert LS.TWO31 % P != 0 and LS.TWO32 % P != 0
    assert G.IQ_P % LS.IQ_CHUNK == 0 and G.IQ_TOTAL == LS.TWO32 + (1 << 20)
    for N in G.SCAN_NFFT:
        assert G.SCAN_P % (N // 2) == 0


def test_iq_expected_totals():
    rng = np.random.default_rng(4)
    v = rng.integers(-128, 128, size=(3 * 4096, 2)).astype(np.int64)
    n_total = 7 * len(v) + 1000
    want = LS.iq_int_sums(np.concatenate([np.tile(v, (7, 1)), v[:1000]]))
    assert LS.iq_expected_int(v, n_total) == [float(n_total)] + [float(w) for w in want]
    with pytest.raises(AssertionError):                          # full-scale s16 does not stay exact for 2^32 samples
        LS.iq_expected_int(np.full((4096, 2), 32767, np.int64), LS.TWO32)
    # the cf32 totals: np.cumsum is the plain loop, bit for bit
    sums = rng.standard_normal((5, 5)) * 1e3
    total = np.zeros(5)
    for c in range(23):
        total = total + sums[c % 5]
    got = LS.iq_expected_cf32(sums, 23)
    assert np.array_equal(got.view(np.uint64), total.view(np.uint64))
