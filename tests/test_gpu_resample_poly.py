"""The audio resampler's polyphase method (k_resample_poly) bit for bit against the C restatement of its definition
(tests/cpp/resample_poly_ref.c, proven against float64 in test_resample_cpu.py), at every ratio, tap count and call shape, and the
resampler's remaining entries.  What each test is for, by the gaps it closes:
  1  history assembled from history (calls shorter than T - 1 behind live data)      test_call_shapes_over_a_live_history
  2  calls that emit nothing (a decimator's short calls)                            test_call_shapes_over_a_live_history
  3  tiles below 256 (128 at 32000 -> 4000, 32 at 32000 -> 1000 with T = 256)       test_every_ratio_and_tap_count
  4  22050, 8000, 4000, 192000, fs_in = 48000                                       test_every_ratio_and_tap_count
  5  taps_per_phase 8 and 256                                                       test_every_ratio_and_tap_count
  6  set_input_rate with an actual change, and a refused one                        test_set_input_rate_*
  7  strides, views, exact and short outputs, refused sizes                         test_strides_views_and_refused_calls_*
  8  reset(c) and reset(-1) are right, not merely different                         test_reset_one_channel_then_all
  9  NaN, infinities, overflow, denormals, signed zeros; pcm16 past 16 bits         test_non_finite_and_extreme_samples, test_pcm16_wraps_past_16_bits
  10 the reference method's table cache past its 32 entries                         test_reference_method_table_cache
  11 the host-destination entry: scratch growth, n_out = 0                          test_host_destination_entry
Everything is compared as bits; two NaNs in the same place count as equal.  Every f32 comparison is repeated for process_pcm16 on a
second handle fed the same calls, against the restatement's pcm16 (values it reports as unspecified are skipped)."""
import ctypes as C

import numpy as np
import pytest

import resample_ref
from conftest import describe_diff
from resample_ref import POLY_CASES, noise_and_tone, poly_call_shapes, poly_count, poly_three_calls

pytestmark = pytest.mark.gpu
F_SENT, P_SENT = 7.25, 12345          # what the output tensors hold before a call
ERR_ARG, ERR_SIZE = -1, -2


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def PolyRef(tmp_path_factory):
    return resample_ref.build_poly(tmp_path_factory.mktemp("resample_poly_ref_gpu"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return resample_ref.build(tmp_path_factory.mktemp("resample_ref_gpu_poly"))


def same(a: np.ndarray, b: np.ndarray) -> bool:
    """the same bits, NaNs place for place"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(b)
    return bool(np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


class CopyRef:
    """equal rates: a call passes its input through"""
    def __init__(self):
        self.pos = 0

    def output_frames(self, k):
        return k

    def counters(self):
        return self.pos, self.pos

    def process(self, x):
        self.pos += x.shape[1]
        return np.ascontiguousarray(x, np.float32).copy()


class Pair:
    """one stream through the library twice (an f32 handle and a pcm16 handle) and through the restatement"""
    def __init__(self, f, p, ref, L, M, PolyRef):
        self.f, self.p, self.ref, self.L, self.M, self.PolyRef = f, p, ref, L, M, PolyRef

    def reset(self, channel=-1):
        for o in (self.f, self.p, self.ref):
            o.reset(channel)


def make_pair(pkg, PolyRef, n_channels, fs_out, fs_in=32000, tpp=0, max_in=1 << 16):
    taps, L, M = pkg.resampler_design(fs_in, fs_out, taps_per_phase=tpp)
    f, p = (pkg.AudioResampler(n_channels, fs_out, fs_in=fs_in, taps_per_phase=tpp, max_input_frames=max_in) for _ in range(2))
    return Pair(f, p, PolyRef(n_channels, L, M, taps), L, M, PolyRef)


def check(pair, y, p, e, what):
    assert same(y, e), (what, describe_diff(y, e))
    ep, un = pair.PolyRef.pcm16(e)
    assert p.shape == ep.shape and np.array_equal(p[~un], ep[~un]), (what, int((p[~un] != ep[~un]).sum()))


def run_calls(pair, x, splits, streams=(None,), what=""):
    """Feeds x [C, sum(splits), 2] in calls of `splits` frames, each the head of a view into one device tensor, into outputs 3 frames wider than the
    call needs and prefilled with a sentinel.  Before each call output_frames equals the restatement's count; after all of them (one
    synchronisation) every call's f32 and pcm16 equal the restatement and the sentinels stand.  Returns the device's f32 outputs."""
    import torch
    n_ch = x.shape[0]
    assert x.shape[1] == sum(splits)
    xd = torch.from_numpy(np.concatenate([x, np.full((n_ch, 1, 2), np.nan, np.float32)], axis=1)).cuda()   # (one frame no call may read)
    pos = pair.ref.counters()[0]
    wants = []
    for k in splits:
        wants.append(poly_count(pos, k, pair.L, pair.M))
        pos += k
    outs = [(torch.full((n_ch, w + 3, 2), F_SENT, dtype=torch.float32, device="cuda"), torch.full((n_ch, w + 3, 2), P_SENT, dtype=torch.int16, device="cuda"))
            for w in wants]
    torch.cuda.synchronize()
    at, exp = 0, []
    for i, (k, w) in enumerate(zip(splits, wants)):
        s = streams[i % len(streams)]
        assert pair.ref.output_frames(k) == w and pair.f.output_frames(k) == w and pair.p.output_frames(k) == w, (what, i, k, w)
        xv = xd[:, at:]                                  # the rest of the tensor: the call reads its first k frames
        y = pair.f.process(xv, n_in=k, out=outs[i][0], stream=s)
        p = pair.p.process_pcm16(xv, n_in=k, out=outs[i][1], stream=s)
        assert y.shape[1] == w and p.shape[1] == w, (what, i)
        exp.append(pair.ref.process(x[:, at:at + k]))
        at += k
    torch.cuda.synchronize()
    got = []
    for i, w in enumerate(wants):
        y, p = outs[i][0].cpu().numpy(), outs[i][1].cpu().numpy()
        check(pair, y[:, :w], p[:, :w], exp[i], (what, "call", i, "frames", splits[i]))
        assert np.all(y[:, w:] == np.float32(F_SENT)) and np.all(p[:, w:] == P_SENT), (what, "sentinel", i)
        got.append(y[:, :w].copy())
    return got, wants


CASE_C = [(c, 5) for c in sorted(POLY_CASES)] + [((32000, 44100, 0), 1), ((32000, 44100, 0), 4), ((32000, 4000, 0), 1), ((32000, 4000, 0), 4)]


@pytest.mark.parametrize("case,n_channels", CASE_C, ids=[f"{c[0]}-{c[1]}-T{c[2]}-C{n}" for c, n in CASE_C])
def test_every_ratio_and_tap_count(pkg, PolyRef, case, n_channels):
    """Gaps 3, 4, 5.  Every ratio and tap count of POLY_CASES (their (L, M, T, tile) asserted in test_resample_cpu.py: tile 128 at 4000,
    tile 32 at 1000) with C = 5, a full station group and a ragged one, and C = 1 and 4 for two of them.  Three calls: two full tiles and a
    ragged third, one tile, fewer than 64 outputs."""
    L, M, T, tile = POLY_CASES[case]
    pair = make_pair(pkg, PolyRef, n_channels, case[1], fs_in=case[0], tpp=case[2])
    assert (pair.L, pair.M, pair.ref.T) == (L, M, T)
    calls = poly_three_calls(L, M, tile)
    x = noise_and_tone(n_channels, sum(calls), seed=11, fs_in=case[0])
    _, wants = run_calls(pair, x, calls, what=case)
    assert 2 * tile + 17 <= wants[0] < 3 * tile and tile <= wants[1] < tile + 64 and 0 < wants[2] < 64
    if L <= M:
        assert wants[:2] == [2 * tile + 17, tile]


@pytest.mark.parametrize("fs_out", [44100, 22050, 8000, 4000])
def test_call_shapes_over_a_live_history(pkg, PolyRef, fs_out):
    """Gaps 1 and 2.  Behind 3 T frames of data: calls of 1, 1, 1, 0, 2, T - 2, T - 1, T, T + 1, 1, 5 T + 3, 1, 1 frames, alternating between
    two streams with no host synchronisation.  The short ones assemble the next history from the history itself; at 8000 and 4000 several
    emit nothing and still have to hand the history over.  n = 0 and zero-output calls leave their sentinel-filled outputs untouched."""
    import torch
    pair = make_pair(pkg, PolyRef, 5, fs_out)
    T = pair.ref.T
    splits = [3 * T] + poly_call_shapes(T)
    x = noise_and_tone(5, sum(splits), seed=12)
    _, wants = run_calls(pair, x, splits, streams=(torch.cuda.Stream(), torch.cuda.Stream()), what=fs_out)
    assert splits[4] == 0 and wants[4] == 0
    if fs_out in (8000, 4000):
        assert sum(1 for k, w in zip(splits, wants) if k > 0 and w == 0) >= 3, wants


def _raw(rs, name, x, in_stride, n_in, out, out_stride):
    """the C entry with every argument as given: (status, n_out as the call left it)"""
    import torch
    got = C.c_longlong(-77)
    rc = getattr(rs.L, name)(rs.r, C.c_void_p(x.data_ptr()), in_stride, n_in, C.c_void_p(out.data_ptr()), out_stride, C.byref(got),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, got.value


def _strides_and_refusals(pkg, rs_f, rs_p, expect, fs_out, check_out):
    """What the two methods' stride tests share.  rs_f / rs_p: handles of 5 channels with max_input_frames 256, fed the same calls;
    expect(x [C, n, 2]) -> the call's expected f32 output; check_out(y, p, e, what) compares."""
    import torch
    n_ch, width, n_in = 5, 301, 200
    seg = [noise_and_tone(n_ch, n_in, seed=13 + i) for i in range(3)]
    entries = ((rs_f, "process", "fmd_resampler_process_f32_dev", torch.float32, F_SENT), (rs_p, "process_pcm16", "fmd_resampler_process_pcm16_dev", torch.int16, P_SENT))

    def wide_input(x):
        # rows of 301 frames (an odd count: rows 8-byte aligned only), the view starts at frame 1, NaN in every frame the call must not read
        w = np.full((n_ch, width, 2), np.nan, np.float32)
        w[:, 1:1 + n_in] = x
        return torch.from_numpy(w).cuda()[:, 1:281]

    def call(x, extra):
        """one valid call of both handles: out `extra` frames wider than n_out"""
        e = expect(x)
        w = e.shape[1]
        res = []
        for rs, meth, _, dtype, sent in entries:
            assert rs.output_frames(n_in) == w
            out = torch.full((n_ch, w + extra, 2), sent, dtype=dtype, device="cuda")
            y = getattr(rs, meth)(wide_input(x), n_in=n_in, out=out)
            assert y.shape[1] == w
            o = out.cpu().numpy()
            assert np.all(o[:, w:] == np.asarray(sent, o.dtype)), "sentinel"
            res.append(o[:, :w])
        assert not np.isnan(res[0]).any()
        check_out(res[0], res[1], e, ("valid call, out wider by", extra))

    call(seg[0], 4)             # out wider than n_out
    call(seg[1], 0)             # out of exactly n_out frames
    # refused calls: FMD_ERR_SIZE, nothing written, nothing advanced
    w = rs_f.output_frames(n_in)
    for rs, meth, cname, dtype, sent in entries:
        xin = wide_input(seg[2])
        out = torch.full((n_ch, w + 2, 2), sent, dtype=dtype, device="cuda")
        assert _raw(rs, cname, xin, width, n_in, out, w - 1) == (ERR_SIZE, -77)                 # out one frame short
        big = torch.full((n_ch, 300, 2), 0.5, dtype=torch.float32, device="cuda")
        out2 = torch.full((n_ch, 800, 2), sent, dtype=dtype, device="cuda")
        with pytest.raises(pkg.FmdError) as err:                                                 # n_in > max_input_frames
            getattr(rs, meth)(big, n_in=257, out=out2)
        assert err.value.status == ERR_SIZE
        with pytest.raises(pkg.FmdError) as err:                                                 # n_in > in_stride
            getattr(rs, meth)(big[:, :100].contiguous(), n_in=101, out=out)
        assert err.value.status == ERR_SIZE
        assert _raw(rs, cname, xin, n_in - 1, n_in, out, w + 2) == (ERR_SIZE, -77)
        torch.cuda.synchronize()
        assert bool((out == sent).all()) and bool((out2 == sent).all()), meth
        assert rs.output_frames(n_in) == w
    call(seg[2], 1)             # the stream continues as if the refused calls had not been made


def test_strides_views_and_refused_calls_polyphase(pkg, PolyRef):
    """Gap 7, polyphase at 44100.  Input: a view from an odd frame of a wider tensor, n_in smaller than the view, NaN everywhere else; out
    wider than n_out (sentinel intact, no NaN), exactly n_out, and one frame short (FMD_ERR_SIZE, nothing written); n_in beyond
    max_input_frames and beyond in_stride likewise.  The valid call behind the refused ones continues the stream bit for bit: no counter
    advanced, no history flipped."""
    pair = make_pair(pkg, PolyRef, 5, 44100, max_in=256)
    _strides_and_refusals(pkg, pair.f, pair.p, pair.ref.process, 44100, lambda y, p, e, what: check(pair, y, p, e, what))


def test_strides_views_and_refused_calls_reference(pkg, PolyRef, ref):
    """Gap 7, the reference method at 44100 against tests/cpp/resample_ref.c: the same views, widths and refusals."""
    f, p = (pkg.AudioResampler(5, 44100, method="reference", max_input_frames=256) for _ in range(2))

    def check_out(y, pq, e, what):
        assert same(y, e), (what, describe_diff(y, e))
        assert np.array_equal(pq, PolyRef.pcm16(e)[0]), what
    _strides_and_refusals(pkg, f, p, lambda x: np.stack([ref(x[c], 44100) for c in range(x.shape[0])]), 44100, check_out)


@pytest.mark.parametrize("calls_before", [1, 2])
@pytest.mark.parametrize("fs_out", [44100, 8000])
def test_reset_one_channel_then_all(pkg, PolyRef, fs_out, calls_before):
    """Gap 8.  C = 6: after 3 T + 7 frames in one call or in two (reset(c) clears the history buffer the next call reads, which alternates),
    reset(2), one more call: every channel equals the restatement after its own reset(2): the others untouched, channel 2 with a zero past
    and the shared counters kept.  Then reset(-1): a fresh stream from counter 0."""
    pair = make_pair(pkg, PolyRef, 6, fs_out)
    T = pair.ref.T
    before = [3 * T + 7] if calls_before == 1 else [T + 3, 2 * T + 4]
    x = noise_and_tone(6, 3 * T + 7 + 2 * T + 5, seed=14)
    run_calls(pair, x[:, :3 * T + 7], before, what="before the reset")
    pair.reset(2)
    assert pair.ref.counters() == (3 * T + 7, -(-(3 * T + 7) * pair.L // pair.M))
    run_calls(pair, x[:, 3 * T + 7:], [2 * T + 5], what="after reset(2)")
    pair.reset(-1)
    assert pair.ref.counters() == (0, 0)
    (y,), _ = run_calls(pair, x[:, :T + 9], [T + 9], what="after reset(-1)")
    fresh = PolyRef(6, pair.L, pair.M, pkg.resampler_design(32000, fs_out)[0]).process(x[:, :T + 9])
    assert same(y, fresh)


@pytest.mark.parametrize("fs_out,rates", [(16000, [32000, 16000, 48000, 32000]), (48000, [32000, 16000, 32000])], ids=["to16000", "to48000"])
def test_set_input_rate_changes_the_filter_and_restarts_the_stream(pkg, PolyRef, fs_out, rates):
    """Gap 6.  One handle, C = 3, data on both sides of every change.  fs_out 16000: 32000 -> 16000 (equal rates: the copy kernel, output
    bits = input bits) -> 48000 (M / L = 3, T 32 -> 96: the histories are re-allocated) -> 32000; fs_out 48000: 32000 -> 16000 (L = 3) ->
    32000.  Each change returns True and a repeat of the rate False; after each, the outputs equal a fresh restatement at the new ratio."""
    f, p = (pkg.AudioResampler(3, fs_out, fs_in=rates[0], max_input_frames=4096) for _ in range(2))
    seen_T = []
    for i, fs_in in enumerate(rates):
        if i > 0:
            assert f.set_input_rate(fs_in) is True and p.set_input_rate(fs_in) is True
        assert f.set_input_rate(fs_in) is False and p.set_input_rate(fs_in) is False
        taps, L, M = pkg.resampler_design(fs_in, fs_out)
        seen_T.append(taps.shape[0])
        pair = Pair(f, p, CopyRef() if fs_in == fs_out else PolyRef(3, L, M, taps), L, M, PolyRef)
        x = noise_and_tone(3, 700 + 333 + 2, seed=20 + i, fs_in=fs_in)
        run_calls(pair, x, [700, 333, 2], what=(fs_in, fs_out))
    assert seen_T == ([64, 32, 96, 64] if fs_out == 16000 else [32, 32, 32])


def test_set_input_rate_refused_leaves_the_stream_alone(pkg, PolyRef):
    """Gap 6.  32000 -> 48000 with 8 taps per phase asked to go to fs_in = 999983 (a prime: M > 4096, which the design refuses): FMD_ERR_ARG,
    and the stream continues bit for bit at the old rate."""
    pair = make_pair(pkg, PolyRef, 3, 48000, tpp=8)
    x = noise_and_tone(3, 500, seed=25)
    run_calls(pair, x[:, :260], [255, 5], what="before")
    for rs in (pair.f, pair.p):
        with pytest.raises(pkg.FmdError) as err:
            rs.set_input_rate(999983)
        assert err.value.status == ERR_ARG and rs.fs_in == 32000
    run_calls(pair, x[:, 260:], [3, 237], what="after the refused change")


def _specials(T, n1):
    """frame -> (left, right) for the channel that carries special samples; n1: length of the first call"""
    return {40: (-0.0, 0.0), 70: (1e-40, -1e-40), 75: (3e-39, -3e-39), 3 * T: (np.inf, 0.25), 3 * T + T // 2: (-0.5, -np.inf),
            6 * T: (1e38, -1e38), 8 * T: (np.nan, 0.125), n1 - 5: (0.5, np.nan)}


@pytest.mark.parametrize("fs_out", [48000, 8000])
def test_non_finite_and_extreme_samples(pkg, PolyRef, fs_out):
    """Gap 9.  C = 8; channel 5 carries +-0, denormals, +-inf, NaN and +-1e38 at known frames, a NaN 5 frames before the end of the first
    call (it reaches the second call through the history), and in the second call a run of +-3e38 signed like one phase's taps, so that
    that output's chain overflows.  f32 equals the restatement, NaNs place for place; outside the outputs whose window [m - T + 1, m]
    holds a non-finite or huge frame the channel is finite; the other seven channels, its three workgroup neighbours included, equal a
    run without the special samples bit for bit."""
    pair, clean = make_pair(pkg, PolyRef, 8, fs_out), make_pair(pkg, PolyRef, 8, fs_out)
    L, M, T = pair.L, pair.M, pair.ref.T
    n1, n2 = 10 * T + 9, 6 * T + 3
    x = noise_and_tone(8, n1 + n2, seed=30)
    xs = x.copy()
    bad = []
    for m, v in _specials(T, n1).items():
        xs[5, m] = v
        if not np.all(np.isfinite(v)) or max(abs(v[0]), abs(v[1])) > 1e30:
            bad.append(m)
    # the overflow: the window of output n0 holds 3e38 sign(h) on the left rail
    taps = pkg.resampler_design(32000, fs_out)[0]
    m0 = n1 + 4 * T
    n0 = -(-m0 * L // M)                        # the first output whose newest frame is m0 or later
    m0, p0 = n0 * M // L, n0 * M % L
    h = taps[:, p0].astype(np.float64)
    assert np.abs(h).sum() * 3e38 > 3.5e38, "this phase's taps cannot overflow the chain"
    for t in range(T):
        xs[5, m0 - t, 0] = 3e38 if h[t] >= 0 else -3e38
        bad.append(m0 - t)
    got, wants = run_calls(pair, xs, [n1, n2], what="special")
    ref_got, _ = run_calls(clean, x, [n1, n2], what="clean")
    y, yc = np.concatenate(got, axis=1), np.concatenate(ref_got, axis=1)
    assert np.isinf(y[5, n0, 0]), "the chain of output n0 was meant to overflow"
    assert np.isnan(y[5, :wants[0]]).any() and np.isnan(y[5, wants[0]:]).any()          # both calls see a NaN: the second through the history
    m = np.arange(y.shape[1], dtype=np.int64) * M // L
    touched = np.zeros(y.shape[1], bool)
    for b in bad:
        touched |= (m - (T - 1) <= b) & (b <= m)
    assert np.isfinite(y[5, ~touched]).all() and (~touched).sum() > 0
    for c in range(8):
        if c != 5:
            assert same(y[c], yc[c]), c


def test_pcm16_wraps_past_16_bits(pkg, PolyRef):
    """Gap 9.  A +-1.0 square wave at 48000: the filter overshoots past 1 / 0.95, so |sample * 31128.65| passes 32768.  pcm16 there is the low
    16 bits of the truncated product (it wraps, as the reference's conversion does), equal to the restatement's."""
    pair = make_pair(pkg, PolyRef, 2, 48000)
    n = 600
    x = np.empty((2, n, 2), np.float32)
    for c in range(2):
        for r in range(2):
            x[c, :, r] = np.where(((np.arange(n) + 3 * c + r) // (8 + 3 * c)) % 2 == 0, 1.0, -1.0)
    got, _ = run_calls(pair, x, [n], what="square wave")
    t = got[0] * (np.float32(32767.0) * np.float32(0.95))
    assert (np.abs(t) >= 32768.0).any() and np.abs(t).max() < 2.0 ** 31
    assert not pair.PolyRef.pcm16(got[0])[1].any()


def test_reference_method_table_cache(pkg, PolyRef, ref):
    """Gap 10.  One reference-method handle at 48000, C = 5, 40 distinct input lengths in 64 ... 2048 in scrambled order: the cache of 32
    index tables fills, is flushed and rebuilt.  Revisits of a cached length, of an evicted one and of one inserted after the flush; a
    length whose index chain leaves the input (16384) in the middle returns FMD_ERR_ARG and writes nothing.  Every call equals
    tests/cpp/resample_ref.c in f32 and pcm16."""
    import torch
    rng = np.random.default_rng(40)
    lengths = [64, 2048] + [int(v) for v in rng.choice(np.arange(65, 2048), 38, replace=False)]
    lengths = [lengths[i] for i in rng.permutation(40)]
    assert len(set(lengths)) == 40 and 16384 not in lengths
    order = lengths[:20] + [lengths[3]] + lengths[20:32] + [16384] + lengths[32:36] + [lengths[5], lengths[33], lengths[3]] + lengths[36:] + [lengths[39], lengths[0]]
    x = noise_and_tone(5, 16384, seed=41)
    xd = torch.from_numpy(x).cuda()
    f, p = (pkg.AudioResampler(5, 48000, method="reference", max_input_frames=16384) for _ in range(2))
    for i, k in enumerate(order):
        if k == 16384:
            for rs, meth, dtype, sent in ((f, "process", torch.float32, F_SENT), (p, "process_pcm16", torch.int16, P_SENT)):
                out = torch.full((5, 24576, 2), sent, dtype=dtype, device="cuda")
                with pytest.raises(pkg.FmdError) as err:
                    getattr(rs, meth)(xd, n_in=k, out=out)
                assert err.value.status == ERR_ARG
                torch.cuda.synchronize()
                assert bool((out == sent).all())
            continue
        y, q = f.process(xd, n_in=k).cpu().numpy(), p.process_pcm16(xd, n_in=k).cpu().numpy()
        e = np.stack([ref(x[c, :k], 48000) for c in range(5)])
        assert same(y, e), (i, k, describe_diff(y, e))
        assert np.array_equal(q, PolyRef.pcm16(e)[0]), (i, k)


def test_host_destination_entry(pkg, PolyRef):
    """Gap 11.  fmd_resampler_process_f32_host at 8000, C = 5: a small call, a larger one (the scratch buffer grows), calls that emit one and
    no frame, and one more; the host array is wider than n_out with a sentinel behind each row.  Equal to the device entry (and the
    restatement) bit for bit."""
    import torch
    pair = make_pair(pkg, PolyRef, 5, 8000)
    host = pkg.AudioResampler(5, 8000)
    splits = [100, 1000, 1, 1, 50]
    x = noise_and_tone(5, sum(splits), seed=50)
    dev, wants = run_calls(pair, x, splits, what="device entry")
    assert wants[0] < wants[1] and 0 in wants[2:4]
    xd = torch.from_numpy(x).cuda()
    at = 0
    for i, (k, w) in enumerate(zip(splits, wants)):
        out = np.full((5, w + 2, 2), F_SENT, np.float32)
        assert host.output_frames(k) == w
        assert host.process_host(xd[:, at:at + k], out) == w
        assert same(out[:, :w], dev[i]), (i, describe_diff(out[:, :w], dev[i]))
        assert np.all(out[:, w:] == np.float32(F_SENT)), i
        at += k
