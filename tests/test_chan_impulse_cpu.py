"""The impulse-train plan of tests/chan_impulse.py, host side (no GPU): the conditions that make the GPU comparison exact hold for every
configuration the GPU tests run, and the plan's expectation is the float64 restatement (test_channelizer.ref_channelize) of the same
impulse train.  These are conditions on the reference side alone."""
import numpy as np
import pytest

import chan_impulse as CI
from test_channelizer import ref_channelize


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


def _design(pkg, fs_in, tpp):
    T = tpp or pkg.chan_default_taps(fs_in, CI.FS_OUT)
    taps, L, M = pkg.chan_design(fs_in, CI.FS_OUT, T)
    return taps, L, M, T


@pytest.mark.parametrize("cfg", CI.CONFIGS, ids=CI.config_id)
def test_preconditions_of_the_exact_comparison(pkg, cfg):
    fs_in, tpp, _, tile = cfg
    taps, L, M, T = _design(pkg, fs_in, tpp)
    for fmt in ("cf32", "u8", "s16"):
        plan = CI.ImpulsePlan(L, M, T, fmt)
        # at most one impulse per window: the impulses are at least T apart, and no output is claimed twice
        assert np.diff(plan.pos).min() >= T and plan.pos[-1] + T <= plan.n_in
        assert np.unique(plan.hit_outputs).size == plan.hit_outputs.size
        n0 = (plan.hit_outputs * M) // L                                  # the newest sample of the output's window
        n_i = plan.pos[plan.hit_impulse]
        assert np.all((n0 - (T - 1) <= n_i) & (n_i <= n0))
        ns = (np.flatnonzero(plan.silent) * M) // L
        j = np.searchsorted(plan.pos, ns, side="right") - 1               # the last impulse at or before a silent output's newest sample
        assert np.all(plan.pos[j] < ns - (T - 1))                         # ... lies in front of its window
        # every residue mod M, so every tap exactly once
        assert np.array_equal(np.sort(plan.pos % M), np.arange(M))
        assert plan.hit_tap.size == L * T and np.array_equal(np.sort(plan.hit_tap), np.arange(L * T))
        n_silent = int(plan.silent.sum())
        assert n_silent >= 1 and n_silent + L * T == plan.n_out
        # amplitudes: 0 or a power of two per component, never both zero, representable in the format
        m, e = np.frexp(np.abs(plan.amp))
        assert np.all((m == 0.5) | (plan.amp == 0)) and np.all(np.abs(plan.amp).max(axis=1) > 0)
        x = plan.input()
        conv = x.astype(np.float64) - (127 if fmt == "u8" else 0)
        assert np.array_equal(conv[plan.pos], plan.amp) and np.count_nonzero(conv) == np.count_nonzero(plan.amp)
        # every expected value a normal float (no subnormal product) or zero, and nothing but zero at the silent outputs
        tiny = np.finfo(np.float32).tiny
        assert np.all(np.abs(taps) >= tiny)
        for q in CI.QUARTERS:
            want = plan.expected_exact(taps, q)
            assert np.all(np.isfinite(want)) and np.all((want == 0) | (np.abs(want) >= tiny))
            assert np.all(want[plan.silent] == 0) and np.all(np.abs(want[~plan.silent]).max(axis=1) > 0)
            # exact: the float32 product is the float64 product
            ho, a, n = plan._per_output(taps)
            prod = np.abs(ho.astype(np.float64)[:, None] * a)             # |h a|, real and imaginary: swapped where (-j)^(q n) is +-j
            swap = ((q * n) % 2 == 1)[:, None]
            assert np.array_equal(np.abs(want).astype(np.float64), np.where(swap, prod[:, ::-1], prod))
        # the call shapes cut at multiples of M and cover the stream; the uneven shape has a call of more than four tiles where it can
        for shape in ("one", "shortest", "uneven"):
            cuts = plan.cuts(shape, tile)
            assert cuts[0] == 0 and cuts[-1] == plan.n_in and all(c % M == 0 for c in cuts) and all(b > a for a, b in zip(cuts, cuts[1:]))
        if plan.n_out >= 6 * tile:
            assert max(b - a for a, b in zip(cuts, cuts[1:])) * L // M > 4 * tile


@pytest.mark.parametrize("fs_in,tpp", [(10e6, 4), (12.8e6, 0)])
def test_expectation_is_the_float64_restatement(pkg, fs_in, tpp):
    """ref_channelize of the impulse train, at the exact centres, at dyadic centres (whose phase f / fs_in * n is exact in float64, as
    the library's increment is) to 1e-12 of the tap, and at the GPU tests' generic centres, to 1e-12 plus the rounding of
    ref_channelize's own phase product (2 pi n_in |f / fs_in| 2^-53 rad)."""
    taps, L, M, T = _design(pkg, fs_in, tpp)
    plan = CI.ImpulsePlan(L, M, T)
    xf = plan.input()
    x = xf[:, 0].astype(np.float64) + 1j * xf[:, 1]
    dyadic = np.array([3 / 16, -5 / 32, 1 / 1024]) * fs_in
    cs = CI.centers(fs_in)
    for k, f in enumerate(np.concatenate([cs, dyadic])):
        ref = ref_channelize(x, f, taps, L, M, fs_in=fs_in)
        got, scale = plan.expected_float64(taps, f, fs_in)
        assert ref.shape == got.shape
        assert np.all(ref[plan.silent] == 0) and np.all(got[plan.silent] == 0)
        tol = 1e-12 + (2 * np.pi * plan.n_in * abs(f / fs_in) * 2.0 ** -53 if 3 <= k < 6 else 0.0)
        hit = ~plan.silent
        assert np.all(np.abs(got[hit] - ref[hit]) <= tol * scale[hit]), (f, float(np.max(np.abs(got[hit] - ref[hit]) / scale[hit])))
        if k < 3:
            want = plan.expected_exact(taps, CI.QUARTERS[k]).astype(np.float64)
            assert np.all(np.abs(want[hit, 0] + 1j * want[hit, 1] - ref[hit]) <= 1e-12 * scale[hit])


def test_the_checkers_reject_a_dropped_edge_tap_and_a_shift(pkg):
    taps, L, M, T = _design(pkg, 10e6, 4)
    plan = CI.ImpulsePlan(L, M, T)
    first = int(np.flatnonzero(plan.out_tap == 0)[0])                     # the output that shows the prototype's first tap
    want = plan.expected_exact(taps, 1)
    CI.check_exact(want.copy(), want)
    ref, scale = plan.expected_float64(taps, 1234.5, 10e6)
    y = np.stack([ref.real, ref.imag], axis=-1).astype(np.float32)
    assert CI.check_bounded(y, ref, scale) < 1e-7                         # (float32 rounding of the reference itself)
    for mutate in (lambda v: _zeroed(v, first), lambda v: np.roll(v, 1, axis=0)):
        with pytest.raises(AssertionError):
            CI.check_exact(mutate(want), want)
        with pytest.raises(AssertionError):
            CI.check_bounded(mutate(y), ref, scale)
    bad = want.copy()
    bad[first, 0] = np.nan
    with pytest.raises(AssertionError):
        CI.check_exact(bad, want)
    with pytest.raises(AssertionError):
        CI.check_bounded(bad, ref, scale)


def _zeroed(v, at):
    v = v.copy()
    v[at] = 0
    return v
