"""The channeliser's impulse-train plan (tests/test_gpu_channelizer_impulse.py; its preconditions are checked on the CPU by
tests/test_chan_impulse_cpu.py).

By the definition in fmd_channelizer.hip's header, one impulse a at absolute input sample n_i gives, for station k,
    y_k[o] = h[o M - L n_i] a exp(-j 2 pi f_k n_i / fs_in)        for the outputs o with 0 <= o M - L n_i < L T,
the index into the prototype in [t][p] flattened order (Channelizer.taps().reshape(-1)); every other output is zero.  With M impulses
D >= T + 1 samples apart, gcd(D, M) = 1, at n_i = i D:
  * an output's window of T samples holds at most one impulse, so every output of the stream is ONE product or exactly zero;
  * the positions run over every residue mod M, so every one of the L T taps shows in exactly one output — and the impulses fall on the
    last sample of a call, the first of the next, the oldest history sample and the one just dropped when the calls are M samples long.
The stream is n_in = M D samples, n_out = L D outputs.

Exact centres (0, +fs_in / 4, -fs_in / 4: the mixer's phasor is 1, -j, -1 or j exactly) with amplitudes whose components are 0 or a
power of two: every product is exact and every sum in every kernel form adds one non-zero term to zeros, so the expectation is the
library's own float32 tap times the rotated amplitude, compared with == (no tolerance).  Any other centre: the float64 product with
the phase taken from the 64-bit increment as fmd_chan_create quantises it, bound per output relative to that output's own tap,
|y - ref| <= B |h| |a|.
"""
from math import gcd

import numpy as np

from long_stream_ref import library_phase_inc

FS_OUT = 256_000.0

# The bound of the generic centres, per output and relative to its tap: the error of the mixer's fp32 phasor.  A thread's phasor is exact
# (to float) at its first sample and advanced by one complex multiplication per 256 samples; the step's phase is the 32-bit phase rounded
# to float, off by up to 2^-24 pi = 1.9e-7 rad, the same at every step, so the error grows by up to that per step: 22 - 24 steps in the
# 5.6 - 6.0 k-sample windows at 10 MSa/s (up to 4.5e-6), at most 15 steps in the band form's batches of 16 (up to 3e-6).
# Measured on an MI355X over every configuration, format and call shape of the GPU tests: worst 4.18e-6 (10 MSa/s, 1024 taps per phase,
# one call); 3.8 - 4.0e-6 at the other 10 MSa/s tap counts from 512 up, <= 3.3e-6 elsewhere, <= 2.7e-6 on the band form.  B is twice
# the worst, rounded up to two digits.
B_GENERIC = 8.4e-6

# (fs_in, taps per phase (0: the default), Channelizer.form, Channelizer.tile_outputs)
CONFIGS = [
    (10e6, 4, "k_channelize16_mfma", 128),           # the smallest band
    (10e6, 512, "k_channelize16_mfma", 128),
    (10e6, 640, "k_channelize16_mfma", 128),
    (10e6, 644, "k_channelize16_mfma", 128),         # the largest: K = 1229 of 1232
    (10e6, 648, "k_channelize", 128),                # the first tap count past the matrix-core operand that is no multiple of 64
    (10e6, 704, "k_channelize16", 128),
    (10e6, 1024, "k_channelize16", 128),             # kMaxSlice full
    (2.4e6, 0, "k_channelize", 128),                 # L = 8
    (12.8e6, 0, "k_channelize", 128),                # L = 1
    (260e3, 640, "k_channelize", 128),               # L = 64, M = 65: the largest L
    (25e6, 0, "k_channelize", 32),
    (20e6, 4096, "k_channelize", 32),
    (16e6, 0, "k_channelize_band_mfma", 128),        # G = 8
    (20.48e6, 0, "k_channelize_band_mfma", 128),
    (20e6, 0, "k_channelize_band_mfma", 64),         # G = 4
    (24e6, 0, "k_channelize_band_mfma", 64),
    (30.72e6, 0, "k_channelize_band_mfma", 64),
    (32e6, 0, "k_channelize_band_mfma", 64),
    (32.768e6, 0, "k_channelize_band_mfma", 64),
    (32.768e6, 3000, "k_channelize_band_mfma", 32),  # G = 2
    (32.768e6, 4096, "k_channelize_band_mfma", 32),
]


def config_id(cfg):
    fs_in, tpp, form, tile = cfg
    return f"{fs_in / 1e6:g}M-{tpp or 'default'}-{form}-{tile}"


QUARTERS = (0, 1, -1)                                # the exact centres, in units of fs_in / 4


def centers(fs_in):
    """the six rows of a test handle: the three exact centres, then three generic ones"""
    return np.concatenate([np.array(QUARTERS) * (fs_in / 4.0), np.linspace(-0.45, 0.45, 3) * fs_in + 1234.5])


# the powers of two an impulse's components take, per format (u8: as the converted value v - 127)
_EXPONENTS = {"cf32": (-2, 2), "u8": (0, 6), "s8": (0, 6), "s16": (0, 14)}
_DTYPES = {"cf32": np.float32, "u8": np.uint8, "s8": np.int8, "s16": np.int16}


class ImpulsePlan:
    """Positions, amplitudes and, per output, the impulse and the prototype index it shows (-1: a silent output)."""

    def __init__(self, L, M, T, fmt="cf32", seed=1):
        assert gcd(L, M) == 1
        self.L, self.M, self.T, self.fmt = L, M, T, fmt
        D = T + 1
        while gcd(D, M) != 1:
            D += 1
        self.D = D
        self.n_in, self.n_out = M * D, L * D
        self.pos = np.arange(M, dtype=np.int64) * D
        # amplitudes: each component 0 or +-2^k, never both zero; real-only, imaginary-only and full impulses in turn
        rng = np.random.default_rng(seed)
        lo, hi = _EXPONENTS[fmt]
        comp = np.ldexp(rng.choice([-1.0, 1.0], size=(M, 2)), rng.integers(lo, hi + 1, size=(M, 2)))
        kind = rng.integers(0, 3, size=M)
        comp[kind == 0, 1] = 0.0
        comp[kind == 1, 0] = 0.0
        self.amp = comp                                                   # [M, 2] float64, exact
        # impulse i shows in the outputs o with L n_i <= o M < L n_i + L T
        o_lo = -(-(L * self.pos) // M)
        o_hi = np.minimum(-(-(L * self.pos + L * T) // M), self.n_out)
        cnt = o_hi - o_lo
        imp = np.repeat(np.arange(M), cnt)
        o = np.repeat(o_lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        self.hit_outputs, self.hit_impulse, self.hit_tap = o, imp, o * M - L * self.pos[imp]
        self.out_impulse = np.full(self.n_out, -1, np.int64)
        self.out_tap = np.full(self.n_out, -1, np.int64)
        self.out_impulse[o] = imp
        self.out_tap[o] = self.hit_tap
        self.silent = self.out_tap < 0

    def input(self):
        """the capture, [n_in, 2] interleaved I, Q of the plan's format: zero (u8: 127) except at the impulses"""
        dt = _DTYPES[self.fmt]
        x = np.full((self.n_in, 2), 127 if self.fmt == "u8" else 0, dt)
        x[self.pos] = (self.amp + (127 if self.fmt == "u8" else 0)).astype(dt)
        return x

    def _per_output(self, taps):
        """(tap [n_out] as the library holds it, amplitude [n_out, 2], position [n_out]) of every output; zeros at the silent ones"""
        h = np.asarray(taps, np.float32).reshape(-1)
        assert h.size == self.L * self.T
        imp = np.where(self.silent, 0, self.out_impulse)
        ho = np.where(self.silent, np.float32(0), h[np.where(self.silent, 0, self.out_tap)])
        a = np.where(self.silent[:, None], 0.0, self.amp[imp])
        return ho, a, self.pos[imp]

    def expected_exact(self, taps, quarter):
        """[n_out, 2] float32, station centre quarter * fs_in / 4: tap times a (-j)^(quarter n_i), every product exact"""
        ho, a, n = self._per_output(taps)
        e = (quarter * n) % 4                                             # a (-j)^e: (ar, ai), (ai, -ar), (-ar, -ai), (-ai, ar)
        re = np.choose(e, [a[:, 0], a[:, 1], -a[:, 0], -a[:, 1]]).astype(np.float32)
        im = np.choose(e, [a[:, 1], -a[:, 0], -a[:, 1], a[:, 0]]).astype(np.float32)
        want = np.stack([ho * re, ho * im], axis=-1)
        assert want.dtype == np.float32
        return want

    def expected_float64(self, taps, f_hz, fs_in):
        """(ref [n_out] complex128, scale [n_out] = |h| |a|) for any centre: the phase of impulse i is frac(n_i inc / 2^64) turns with
        inc the library's 64-bit increment, in Python integers"""
        ho, a, _ = self._per_output(taps)
        inc = library_phase_inc(f_hz, fs_in)
        turns = np.array([((int(n) * inc) % (1 << 64)) / float(1 << 64) for n in self.pos], np.float64)
        ph = np.where(self.silent, 0.0, turns[np.where(self.silent, 0, self.out_impulse)])
        ac = a[:, 0] + 1j * a[:, 1]
        return ho.astype(np.float64) * ac * np.exp(-2j * np.pi * ph), np.abs(ho.astype(np.float64)) * np.abs(ac)

    def cuts(self, shape, tile_outputs=128):
        """the call boundaries, in input samples, of a call shape: "one" call; the "shortest" legal calls, M inputs each; "uneven" cuts
        at multiples of M with one call of more than four tiles (where the stream has that many)"""
        D, M = self.D, self.M
        if shape == "one":
            units = [D]
        elif shape == "shortest":
            units = [1] * D
        else:
            big = min(-(-9 * tile_outputs // (2 * self.L)) + 1, D - 7)
            units = [1, 2, big, 1, 3, D - 7 - big] if big >= 1 and D - 7 - big >= 1 else [1, 2, D - 3]
        assert sum(units) == D and min(units) >= 1
        return [int(c) * M for c in np.concatenate([[0], np.cumsum(units)])]


def check_exact(y, want):
    """y, want [n_out, 2] float32: equal value for value (-0 == +0; a NaN equals nothing)"""
    y = np.asarray(y)
    assert y.dtype == np.float32 and want.dtype == np.float32 and y.shape == want.shape, (y.dtype, y.shape, want.shape)
    bad = np.flatnonzero((y != want).any(axis=-1))
    assert bad.size == 0, f"{bad.size} outputs differ, first at {bad[:8].tolist()}: got {y[bad[:4]].tolist()}, expected {want[bad[:4]].tolist()}"


def worst_ratio(y, ref, scale):
    """max over the outputs that show a tap of |y - ref| / (|h| |a|); the silent outputs must be exactly zero"""
    y = np.asarray(y)
    assert y.dtype == np.float32 and y.shape == ref.shape + (2,), (y.dtype, y.shape, ref.shape)
    yc = y[:, 0].astype(np.float64) + 1j * y[:, 1]
    hit = scale > 0
    loud = np.flatnonzero(~hit & ~(yc == 0))
    assert loud.size == 0, f"{loud.size} silent outputs are not zero, first at {loud[:8].tolist()}"
    return float(np.max(np.abs(yc[hit] - ref[hit]) / scale[hit]))


def check_bounded(y, ref, scale, bound=B_GENERIC):
    w = worst_ratio(y, ref, scale)
    assert w <= bound, f"worst |y - ref| / (|h| |a|) = {w:.3e} > {bound:.3e}"      # (a NaN fails the comparison)
    return w
