"""Helpers of the long-stream tests (tests/test_gpu_long_streams.py, checked on the CPU by tests/test_long_stream_ref_cpu.py): the same
device buffer of P samples fed over and over is the signal x[n mod P], known at every absolute index, so the sample counters of the
channeliser, the resampler, the IQ corrector and the band scanner can be driven past 2^31 and 2^32 in seconds.

  * ref_channelize_at: test_channelizer.ref_channelize restated for a start index n0, phase from exact integer arithmetic;
  * chan_period / ChanCase: the choice of the period P and its conditions, as assertions;
  * library_phase_inc: the library's rounding rule for a station's phase increment;
  * iq_expected_int / iq_expected_cf32: the IQ corrector's totals after a periodic stream.
"""
from fractions import Fraction

import numpy as np

TWO31, TWO32 = 1 << 31, 1 << 32
GRID = 4096            # outputs: a multiple of every kernel form's tile (16 ... 128 outputs) and group (16 outputs)
HALF = 192             # outputs compared on each side of a crossing
FS_OUT = 256_000


def ref_channelize_at(x_period, n0, n_out, f, fs_in, taps, L, M):
    """float64 restatement of the channeliser on the stream x[n] = x_period[n mod P] (n >= 0; zero before), for the n_out outputs from
    o0 = n0 L / M on (n0: an absolute input index with a whole o0):
        y[o] = sum_t taps[t, p] x[nc - t] e^{-j 2 pi frac((nc - t) f / fs_in)},  nc = floor(o M / L),  p = (o M) mod L.
    The phase comes from exact integer arithmetic, ((n f_num) mod f_den) / f_den with f / fs_in = f_num / f_den in lowest terms: the
    float64 product f / fs_in * n loses 3e-6 rad at n = 2^32."""
    x_period = np.asarray(x_period, np.complex128)
    P, T = x_period.size, taps.shape[0]
    n0 = int(n0)
    assert n0 >= 0 and (n0 * L) % M == 0, "n0 must be the input index of a whole output"
    q = np.arange(n_out, dtype=np.int64)                       # o = o0 + q and o0 M = n0 L: nc = n0 + floor(q M / L), p = (q M) mod L
    nc_rel, p = (q * M) // L, (q * M) % L
    n_first = n0 - (T - 1)                                     # absolute index of the first sample any of the outputs reads
    span = int(nc_rel[-1]) + T
    i = np.arange(span, dtype=np.int64)
    xs = x_period[((n_first % P) + i) % P]
    if n_first < 0:
        xs = np.where(i < -n_first, 0.0, xs)
    fr = Fraction(f) / Fraction(fs_in)                         # (floats are binary fractions: exact)
    num, den = fr.numerator % fr.denominator, fr.denominator
    r0 = (n_first * num) % den                                 # Python integers: no overflow at any n
    if span * num < (1 << 62):
        turns = ((r0 + i * num) % den).astype(np.float64) / float(den)
    else:
        turns = np.array([((r0 + k * num) % den) / den for k in range(span)], np.float64)
    xm = xs * np.exp(-2j * np.pi * turns)
    idx = (nc_rel + (T - 1))[:, None] - np.arange(T)[None, :]
    return (xm[idx] * taps.astype(np.float64)[np.arange(T)[None, :], p[:, None]]).sum(axis=1)


def library_phase_inc(f, fs_in):
    """fmd_chan_create's phase increment of a station, turns * 2^64 per input sample: llround(ldexp(fr, 63)) << 1 with fr = frac(f / fs_in)
    in double"""
    fr = float(f) / float(fs_in)
    fr -= np.floor(fr)
    v = Fraction(fr) * (1 << 63)                               # ldexp is exact
    return (int(np.floor(v + Fraction(1, 2))) << 1) % (1 << 64)    # llround: halves away from zero, v >= 0


def chan_period(L, M, at_least=1_800_000):
    """the period P = GRID (M / L) 3 2^j of at least `at_least` samples: a whole number of GRID outputs per call, and an odd factor"""
    assert (GRID * M) % L == 0
    P = GRID * M // L * 3
    while P < at_least:
        P *= 2
    return P


class ChanCase:
    """One channeliser stream: the rate pair, its period, the stations and the crossings, with the conditions that make the checks mean
    something.  dyadic: (a, k) pairs, stations at f = fs_in a / 2^k; arbitrary: Hz.  crossings: absolute INPUT indices."""

    def __init__(self, fs_in, L, M, dyadic, arbitrary, P=None, crossings=(TWO31, TWO32), wraps=(TWO31, TWO32)):
        self.fs_in, self.L, self.M = float(fs_in), L, M
        self.P = chan_period(L, M) if P is None else P
        self.dyadic = [fs_in * a / (1 << k) for a, k in dyadic]
        self.centers = np.array(self.dyadic + list(arbitrary), np.float64)
        self.n_dyadic = len(dyadic)
        self.crossings = tuple(crossings)
        self.n_out = self.P * L // M                           # outputs per call
        self.n_calls = (max(self.crossings, default=0) + 2 * self.P) // self.P + 1     # n_abs ends beyond the last crossing + 2 P
        P = self.P
        assert (P * L) % M == 0 and self.n_out % GRID == 0, "every call must have the same tile and group partition"
        for (a, k), f in zip(dyadic, self.dyadic):
            assert P % (1 << k) == 0 and abs(f) < fs_in / 2
            assert (library_phase_inc(f, fs_in) * P) % (1 << 64) == 0, "inc P must vanish mod 2^64"
        for w in wraps:
            # a counter truncated to 31 or 32 bits must break the sequence: P may not divide the wrap, and the wrap may not fall on the
            # grid of tiles either, in input samples or in outputs.  (The grid is taken in outputs: every P here is itself a multiple of
            # 4096 samples, and so is 2^32 mod P — 1 048 576 at 20.48 MSa/s — while (2^32 mod P) L / M is not even whole.)
            assert w % P != 0 and ((w % P) * L) % (GRID * M) != 0 and w % self.n_out != 0
        for n_c in self.crossings:
            call, o_rel = self.crossing(n_c)
            assert 0 < call < self.n_calls - 2 and HALF <= o_rel and o_rel + HALF <= self.n_out, "the compared outputs lie in one call"

    def crossing(self, n_c):
        """(call index, output index within that call) of the first output whose newest input sample is at or beyond n_c"""
        call = n_c // self.P
        return call, -(-((n_c - call * self.P) * self.L) // self.M)

    def window(self, n_c):
        """(call, first output within the call, absolute input index n0 of that output's call start, outputs) of the 2 HALF outputs compared
        at crossing n_c: their input windows end before, straddle and start beyond n_c"""
        call, o_rel = self.crossing(n_c)
        return call, o_rel - HALF, call * self.P, 2 * HALF


def chan_outputs_at(case, x_period, n_c, taps, k):
    """station k's float64 outputs of ChanCase.window(n_c)"""
    call, o_lo, n_call, cnt = case.window(n_c)
    L, M = case.L, case.M
    # ref_channelize_at starts at a whole output: start at the call's first output and keep the last cnt
    # (cheaper: start at the largest multiple of L outputs at or before o_lo, whose input index is whole)
    skip = o_lo % L
    o_start = o_lo - skip
    n0 = n_call + o_start * M // L
    assert (o_start * M) % L == 0
    return ref_channelize_at(x_period, n0, skip + cnt, case.centers[k], case.fs_in, taps, L, M)[skip:]


# ---- the IQ corrector

IQ_CHUNK = 4096


def iq_int_sums(v):
    """v [n, 2] converted integer samples (int64): the five sums as Python integers"""
    i, q = v[:, 0].astype(np.int64), v[:, 1].astype(np.int64)
    return [int(s) for s in (i.sum(), q.sum(), (i * i).sum(), (q * q).sum(), (i * q).sum())]


def iq_expected_int(v_period, n_total):
    """[n, sum i, sum q, sum i^2, sum q^2, sum i q] as doubles after n_total samples of the stream v_period[n mod P]: periods x period sums +
    remainder in Python integers.  Asserts that every partial sum on the way is an integer below 2^53, i.e. that fp64 sums are exact."""
    P = len(v_period)
    periods, rem = divmod(int(n_total), P)
    full, part = iq_int_sums(v_period), iq_int_sums(v_period[:rem])
    tot = [periods * a + b for a, b in zip(full, part)]
    # every partial sum of every moment, in any order, is bounded by the larger of the two sums of squares: |i| <= i^2 for integers, and
    # sum |i q| <= (sum i^2 + sum q^2) / 2
    assert max(tot[2], tot[3]) < (1 << 53) and n_total < (1 << 53)
    return [float(n_total)] + [float(t) for t in tot]


def iq_expected_cf32(chunk_sums, n_chunks):
    """chunk_sums [P / 4096, 5]: the chunk sums of one period (the restatement's moments of each chunk).  The running totals after n_chunks
    chunks of the periodic stream: chunk sums added in chunk order in fp64, starting from +0 (np.cumsum adds sequentially)."""
    chunk_sums = np.asarray(chunk_sums, np.float64)
    reps = -(-n_chunks // len(chunk_sums))
    return np.cumsum(np.tile(chunk_sums, (reps, 1))[:n_chunks], axis=0)[-1]
