"""Sample counts past 2^31 and 2^32 in the four objects that compute with an absolute sample index: the channeliser (mixer phase
frac(n f / fs), polyphase branch (o M) mod L, window start o M / L, tile grouping), the polyphase resampler, the IQ corrector (moments in
4096-sample chunks taken in absolute order) and the band scanner (frame f = samples [f H, f H + N)).  A 20.48 MSa/s capture passes sample
2^32 after 210 s; the other kernel tests stay below 6e4 and the end-to-end tests below 1e7.

One device buffer of P samples is fed over and over, so the input is x[n mod P] at every absolute index (tests/long_stream_ref.py, whose
conditions on P tests/test_long_stream_ref_cpu.py checks without a GPU), through the public API only:
  A. bit-periodicity.  A station at a dyadic offset f / fs = a / 2^k has an exact phase increment inc, and with 2^k | P, inc P = 0 mod
     2^64; with a whole number of 4096 outputs per call every call has the same tiles, windows, seed phases, branches and summation order
     as the one before.  So every call from the second on equals the second bit for bit — unless an index is truncated somewhere: P
     divides neither 2^31 nor 2^32 and the wrap falls on no tile boundary.
  B. the float64 definition at the crossings, for every station (one at an arbitrary offset): the 384 outputs around the first whose
     window reaches sample 2^31 (2^32), against long_stream_ref.ref_channelize_at with the phase from exact integer arithmetic, at the
     bar the kernel tests use at index 0, max|y - ref| / max|ref| < 2e-5.
A alone does not see an index truncated to 32 bits in the mixer's phase: at a dyadic offset with k <= 32, 2^32 inc = 0 mod 2^64.  B's
station at an arbitrary offset does (tried once on a scratch build with n cut to 32 bits in stage_mixed's seed phase: A passed, B gave
1.67 at n = 2^32 for k_channelize16).  The reverse holds for an index cut in a window start or a tile: A covers every output of every
call, B 384 at each crossing.
Input indices only: o_abs stays below 2^32 in the six forms' cases (their streams end between o = 4.4e7 and 4.6e8);
test_channeliser_output_index_past_2_32 carries the OUTPUT index of the 2.4 MSa/s form past 2^32.  There the input index reaches 4e10
and the arbitrary station's error 6.0e-6 (3.0e-6 where o = 2^31): the library's mixer runs at the double frac(f / fs_in), within
2^-54 fs_in of f, and the restatement at the exact f — up to 3.5e-16 rad per sample, 1.4e-5 rad at 4e10 (include/fmdemod.h).

Wall time of each case, measured once on an MI355X (the stream, the checks and the float64 reference on the host), in seconds; none
was reduced, every stream runs past 2^32 + 2 P:
    channeliser, cf32 / integer   k_channelize16_mfma 0.74 / 0.10 (u8)        k_channelize16 0.21 / 0.18 (s8)
                                  k_channelize at 2.4 MSa/s 0.69 / 0.64 (s16)  k_channelize_band_mfma, G = 8 0.27 / 0.25 (u8)
                                  k_channelize_band_mfma, G = 4 0.36 / 0.35 (s8)   k_channelize, tile of 32 0.73 / 0.69 (s16)
    channeliser, output index     4.33 (u8, two stations, 5464 calls of 7 372 800 samples)
    resampler, f32 / pcm16        48 kHz 0.31 / 0.30    44.1 kHz 0.34 / 0.33    16 kHz 0.31 / 0.31
    IQ corrector                  cf32 1.17 (of it 0.02 the stream)    u8 0.15    s8 0.15    s16 0.14
    scanner                       N = 256, s16 1.09    N = 16384, cf32 0.30
"""
import time

import numpy as np
import pytest

import iqcorr_ref
import long_stream_ref as LS
import resample_ref
from long_stream_ref import TWO31, TWO32

pytestmark = pytest.mark.gpu

LIMITS = {"u8": (0, 255, np.uint8), "s8": (-128, 127, np.int8), "s16": (-32768, 32767, np.int16)}


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    return p


def _capture(rng, fmt, n, lo=None, hi=None):
    """[n, 2] of the format: cf32 standard normal; integers over the type's range (or [lo, hi]) with the extremes and zero at the start,
    inside and at the end.  Returns (raw, the cf32 values it stands for as float64 [n, 2])"""
    if fmt == "cf32":
        a = rng.standard_normal((n, 2)).astype(np.float32)
        return a, a.astype(np.float64)
    tlo, thi, dt = LIMITS[fmt]
    lo, hi = tlo if lo is None else lo, thi if hi is None else hi
    a = rng.integers(lo, hi + 1, size=(n, 2)).astype(dt)
    special = np.array([[lo, hi], [hi, lo], [0, 0], [lo, lo], [hi, hi], [0, hi]], dt)
    for at in (0, n // 3, n - len(special)):
        a[at:at + len(special)] = special
    return a, a.astype(np.float64) - (127.0 if fmt == "u8" else 0.0)


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class _Periodic:
    """the bookkeeping of check A on the device: call 0 kept whole, call 1 kept as the pattern, one flag per later call"""

    def __init__(self, n_calls, rows):
        import torch
        self.rows, self.first, self.second = rows, None, None
        self.bad = torch.zeros(n_calls, dtype=torch.bool, device="cuda")

    def add(self, j, y):
        if j == 0:
            self.first = y.clone()
        elif j == 1:
            self.second = y[:self.rows].clone()
        else:
            self.bad[j] = (_bits(y[:self.rows]) != _bits(self.second)).any()

    def check(self, what, P):
        import torch
        bad = torch.nonzero(self.bad).flatten().tolist()
        assert not bad, (f"{what}: {len(bad)} calls differ from the second call, the first of them call {bad[0]} "
                         f"(input samples {bad[0] * P} ... {(bad[0] + 1) * P}; 2^31 is in call {TWO31 // P}, 2^32 in call {TWO32 // P})")
        assert bool(torch.isfinite(self.second.float()).all()) and float(self.second.float().abs().max()) > 0.0
        assert not torch.equal(_bits(self.first[:self.rows]), _bits(self.second))      # (the first call starts from an empty history)


# ---- 1. channeliser: the six rows of test_gpu_channelizer_int.FORMS, each once in cf32 and once in an integer format

# (name, fs_in, taps per phase (0: default), L, M, integer format)
FORMS = [
    ("k_channelize16_mfma", 10e6, 640, 16, 625, "u8"),
    ("k_channelize16", 10e6, 768, 16, 625, "s8"),
    ("k_channelize", 2.4e6, 0, 8, 75, "s16"),
    ("k_channelize_band_mfma, G = 8", 20.48e6, 0, 1, 80, "u8"),
    ("k_channelize_band_mfma, G = 4", 20e6, 0, 8, 625, "s8"),
    ("k_channelize, tile of 32", 25e6, 0, 32, 3125, "s16"),
]
DYADIC = [(3, 5), (-5, 6)]                  # stations at +fs 3 / 32 and -fs 5 / 64


def _arbitrary(fs_in):
    return [round(0.33 * fs_in) + 1234.5]   # the existing tests' "... + 1234.5 Hz" kind


def _case(fs_in, L, M):
    return lambda: LS.ChanCase(fs_in, L, M, DYADIC, _arbitrary(fs_in))


CHAN_CASES = [(f"{name}, {fmt}", _case(fs_in, L, M), fmt) for name, fs_in, tpp, L, M, ifmt in FORMS for fmt in ("cf32", ifmt)]
CHAN_TPP = {f"{name}, {fmt}": tpp for name, fs_in, tpp, L, M, ifmt in FORMS for fmt in ("cf32", ifmt)}


def output_index_case():
    """2.4 MSa/s -> 256 kSa/s (M / L = 9.4, the lowest ratio of the forms): the OUTPUT index passes 2^31 and 2^32 where the input index
    passes 2^31 75 / 8 and 2^32 75 / 8.  One dyadic station and one arbitrary; a period of 7.4 M samples."""
    return LS.ChanCase(2.4e6, 8, 75, DYADIC[:1], _arbitrary(2.4e6), P=LS.chan_period(8, 75, 7_000_000),
                       crossings=(TWO31 * 75 // 8, TWO32 * 75 // 8))


def _stream_channeliser(pkg, name, case, tpp, fmt, seed):
    import torch
    rng = np.random.default_rng(seed)
    raw, conv = _capture(rng, fmt, case.P)
    x_period = conv[:, 0] + 1j * conv[:, 1]
    ch = pkg.Channelizer(case.fs_in, case.centers, max_input_samples=case.P, taps_per_phase=tpp)
    assert (ch.interp, ch.decim) == (case.L, case.M)
    taps = ch.taps()
    xt = torch.from_numpy(raw).cuda()
    out = torch.empty((len(case.centers), case.n_out, 2), dtype=torch.float32, device="cuda")
    per = _Periodic(case.n_calls, case.n_dyadic)
    windows = {case.window(n_c)[0]: n_c for n_c in case.crossings}
    kept = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(case.n_calls):
        y = ch.process(xt, out=out)
        per.add(j, y)
        if j in windows:
            _, o_lo, _, cnt = case.window(windows[j])
            kept[windows[j]] = y[:, o_lo:o_lo + cnt].clone()
    torch.cuda.synchronize()
    t_stream = time.perf_counter() - t0
    assert case.n_calls * case.P > max(case.crossings) + 2 * case.P
    per.check(name, case.P)                                                   # A
    worst = 0.0
    for n_c, y in kept.items():                                               # B
        y = y.cpu().numpy().astype(np.float64)
        for k in range(len(case.centers)):
            ref = LS.chan_outputs_at(case, x_period, n_c, taps, k)
            err = float(np.abs((y[k, :, 0] + 1j * y[k, :, 1]) - ref).max() / np.abs(ref).max())
            print(f"{name}: station {k} ({case.centers[k]:+.1f} Hz) at input sample {n_c}: max|y - ref| / max|ref| = {err:.2e}")
            worst = max(worst, err)
            assert err < 2e-5, (name, k, n_c, err)
    ch.reset()
    again = ch.process(xt, out=out)
    assert torch.equal(_bits(again), _bits(per.first)), name                  # reset: the counters start again at sample 0
    ch.close()
    print(f"{name}: {case.n_calls} calls of {case.P} samples, stream {t_stream:.2f} s, worst error at the crossings {worst:.2e}")


@pytest.mark.parametrize("name,case,fmt", CHAN_CASES, ids=[c[0] for c in CHAN_CASES])
def test_channeliser_past_2_32_input_samples(pkg, name, case, fmt):
    """A on the two dyadic stations in every call, B on all three stations at n = 2^31 and 2^32, then reset() and the first call again"""
    _stream_channeliser(pkg, name, case(), CHAN_TPP[name], fmt, seed=len(name))


def test_channeliser_output_index_past_2_32(pkg):
    """o_abs past 2^31 and 2^32 in k_channelize (u8 input): A on the dyadic station in every call, B on both stations where the output
    index crosses"""
    case = output_index_case()
    assert case.n_calls * case.n_out > TWO32
    _stream_channeliser(pkg, "k_channelize, output index", case, 0, "u8", seed=77)


# ---- 2. polyphase resampler

RS_FS_IN = 32000
RS_P = 320 * 3 * 1024                       # frames per call: whole outputs at every ratio below
RESAMPLE_RATIOS = {48000: (3, 2), 44100: (441, 320), 16000: (1, 2)}
PCM_SCALE = float(np.float32(32767.0) * np.float32(0.95))


@pytest.mark.parametrize("kind", ["f32", "pcm16"])
@pytest.mark.parametrize("fs_out", list(RESAMPLE_RATIOS))
def test_resampler_past_2_32_input_frames(pkg, fs_out, kind):
    """two channels of periodic audio, P frames per call until n_abs > 2^32 + 2 P: every call from the second on equals the second bit for
    bit; the 384 output frames around input frames 2^31 and 2^32 against the float64 restatement (resample_ref.polyphase_f64 over two
    periods: the second period's outputs, whose history is the first period's end) with the bar of
    test_gpu_resample.test_polyphase_against_float64_restatement, 7e-7 (pcm16: the same outputs times 32767 * 0.95f and truncated: within
    1 + 7e-7 * 31129 of the scaled float64 value); fmd_resampler_output_frames against integer arithmetic around each crossing"""
    import torch
    rng = np.random.default_rng(fs_out)
    taps, L, M = pkg.resampler_design(RS_FS_IN, fs_out)
    assert (L, M) == RESAMPLE_RATIOS[fs_out]
    P = RS_P
    n_call = P * L // M
    n_calls = (TWO32 + 2 * P) // P + 1
    t = np.arange(P, dtype=np.float64)
    x = np.clip(0.2 * rng.standard_normal((2, P, 2)), -0.5, 0.5)
    x[0] += 0.4 * np.sin(2 * np.pi * t * 40 / P)[:, None]                     # (whole cycles in a period)
    x[1] += 0.4 * np.sin(2 * np.pi * t * 4321 / P)[:, None]
    x = x.astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    rs = pkg.AudioResampler(2, fs_out, fs_in=RS_FS_IN, max_input_frames=P)
    proc, dtype = (rs.process, torch.float32) if kind == "f32" else (rs.process_pcm16, torch.int16)
    out = torch.empty((2, n_call, 2), dtype=dtype, device="cuda")
    per = _Periodic(n_calls, 2)
    windows, frames_at = {}, set()
    for w in (TWO31, TWO32):
        call = w // P
        o_rel = -(-((w - call * P) * L) // M)
        assert 0 < call < n_calls - 2 and LS.HALF <= o_rel <= n_call - LS.HALF and w % P != 0
        windows[call] = (w, o_rel - LS.HALF)
        frames_at |= {call - 1, call, call + 1}
    kept = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(n_calls):
        if j in frames_at:
            pos = j * P
            for k in (0, 1, 777, P, TWO31 % P + 1, TWO32 % P + 1):
                assert rs.output_frames(k) == -(-(pos + k) * L // M) - -(-pos * L // M), (j, k)
        y = proc(xt, out=out)
        assert y.shape[1] == n_call
        per.add(j, y)
        if j in windows:
            w, o_lo = windows[j]
            kept[w] = y[:, o_lo:o_lo + 2 * LS.HALF].clone()
    torch.cuda.synchronize()
    t_stream = time.perf_counter() - t0
    per.check(f"resampler {fs_out} {kind}", P)
    x2 = np.concatenate([x, x], axis=1).astype(np.float64)
    for w, y in kept.items():
        o_lo = windows[w // P][1]
        y = y.cpu().numpy().astype(np.float64)
        for c in range(2):
            ref = resample_ref.polyphase_f64(x2[c], taps, L, M, n_call + o_lo, n_call + o_lo + 2 * LS.HALF)
            if kind == "f32":
                err = float(np.max(np.abs(y[c] - ref)))
                bar = 7e-7
            else:
                err = float(np.max(np.abs(y[c] - ref * PCM_SCALE)))
                bar = 1.0 + 7e-7 * PCM_SCALE
            print(f"resampler {fs_out} {kind}: channel {c} at input frame {w}: max |err| vs float64 {err:.3e}")
            assert err < bar, (fs_out, kind, c, w, err)
    rs.reset()
    assert torch.equal(_bits(proc(xt, out=out)), _bits(per.first))
    rs.close()
    print(f"resampler {fs_out} {kind}: {n_calls} calls of {P} frames, stream {t_stream:.2f} s")


# ---- 3. IQ corrector

IQ_P = 3 * (1 << 21)                        # a multiple of 4096 that does not divide 2^32
IQ_TOTAL = TWO32 + (1 << 20)
IQ_CORR = (0.37, -1.21, 0.031, -0.047)


@pytest.fixture(scope="module")
def iq_ref(tmp_path_factory):
    return iqcorr_ref.build(tmp_path_factory.mktemp("iqcorr_ref_long"))


@pytest.mark.parametrize("fmt", ["cf32", "u8", "s8", "s16"])
def test_iq_corrector_past_2_32_samples(pkg, iq_ref, fmt):
    """2^32 + 2^20 samples of a periodic capture (the last call a part of a period).  Integer formats: n and the five moments are exactly
    what Python integers give, periods x period sums + remainder — the header's exactness claim (every sum an exact integer below 2^53)
    beyond 2^23 samples; s16 samples span 12 bits (an Airspy's converter), so that 2^32 of them stay below 2^53.  cf32: chunk sums in
    chunk order — the restatement's sums of the period's chunks, added in sequence in fp64 for as many chunks as were streamed — bit for
    bit.  The corrected output of the last call is the first call's."""
    import torch
    rng = np.random.default_rng(31)
    P = IQ_P
    if fmt == "cf32":
        tt = np.arange(P, dtype=np.float64)
        z = 1e-2 * (rng.standard_normal(P) + 1j * rng.standard_normal(P)) + 0.05       # (60 dB of dynamic range and a DC term)
        for f, a in ((0.1234, 10.0), (-0.3071, 3.0), (0.41, 0.01)):
            z = z + a * np.exp(2j * np.pi * ((f * tt) % 1.0))
        raw = np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1).astype(np.float32))
    else:
        raw, conv = _capture(rng, fmt, P, *((-2048, 2047) if fmt == "s16" else ()))
    periods, rem = divmod(IQ_TOTAL, P)
    assert rem > 0 and P % LS.IQ_CHUNK == 0 and IQ_TOTAL % LS.IQ_CHUNK == 0
    xt = torch.from_numpy(raw).cuda()
    co = pkg.IqCorrector(max_input_samples=P)
    co.correction = IQ_CORR
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = co.process(xt).clone()
    for _ in range(periods - 1):
        co.measure(xt)
    last = co.process(xt[:rem])
    got = co.moments()
    t_stream = time.perf_counter() - t0
    assert got.n == float(IQ_TOTAL)
    if fmt == "cf32":
        sums = np.stack([iq_ref.moments(raw[c:c + LS.IQ_CHUNK])[1:] for c in range(0, P, LS.IQ_CHUNK)])
        want = [float(IQ_TOTAL)] + list(LS.iq_expected_cf32(sums, IQ_TOTAL // LS.IQ_CHUNK))
        assert np.array_equal(np.array(got, np.float64).view(np.uint64), np.array(want, np.float64).view(np.uint64)), (list(got), want)
    else:
        want = LS.iq_expected_int(conv.astype(np.int64), IQ_TOTAL)
        assert list(got) == want, (fmt, list(got), want)
    assert torch.equal(_bits(last), _bits(first[:rem]))
    assert not torch.equal(first, xt.float() - (127.0 if fmt == "u8" else 0.0))      # (the correction is not the identity)
    co.close()
    print(f"IQ corrector {fmt}: {periods} calls of {P} samples and one of {rem}, {t_stream:.2f} s")


# ---- 4. band scanner

SCAN_FS = 20_480_000.0
SCAN_P = 3 * (1 << 19)                      # a multiple of every hop
SCAN_NFFT = (256, 16384)


@pytest.mark.parametrize("nfft,fmt", [(256, "s16"), (16384, "cf32")])
def test_scanner_past_2_32_samples(pkg, nfft, fmt):
    """K periods and one hop, K P > 2^32 + P: exactly (n_total - N) / H + 1 = K P / H frames, every one of the P / H frames of the period K
    times.  The PSD equals that of a short run over two periods and one hop (every frame of the period twice) to 1e-9 relative in every
    bin: the fp64 sum of K like terms per frame accounts for the rest."""
    import torch
    rng = np.random.default_rng(nfft)
    P, N, H = SCAN_P, nfft, nfft // 2
    tt = np.arange(P, dtype=np.float64)
    z = 1e-2 * (rng.standard_normal(P) + 1j * rng.standard_normal(P)) + 0.05
    for f, a in ((0.1234, 10.0), (-0.3071, 3.0), (0.41, 0.01)):
        z = z + a * np.exp(2j * np.pi * ((f * tt) % 1.0))
    pairs = np.stack([z.real, z.imag], axis=-1)
    raw = pairs.astype(np.float32) if fmt == "cf32" else np.rint(pairs * 1000.0).astype(np.int16)
    xt = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    K = TWO32 // P + 2
    n_total = K * P + H
    assert P % H == 0 and TWO32 % P != 0 and K * P > TWO32 + P
    sc = pkg.BandScanner(SCAN_FS, nfft=N, max_input_samples=P)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        sc.process(xt)
    sc.process(xt[:H])
    frames = sc.n_frames
    _, got = sc.psd()
    t_stream = time.perf_counter() - t0
    assert frames == (n_total - N) // H + 1 == K * (P // H)
    short = pkg.BandScanner(SCAN_FS, nfft=N, max_input_samples=P)
    short.process(xt)
    short.process(xt)
    short.process(xt[:H])
    assert short.n_frames == 2 * (P // H)
    _, want = short.psd()
    assert np.all(want > 0.0) and np.all(np.isfinite(got))
    rel = float(np.max(np.abs(got - want) / want))
    print(f"scanner N = {N} {fmt}: {frames} frames in {K} calls of {P} samples, {t_stream:.2f} s; PSD against two periods: {rel:.2e} relative")
    assert rel <= 1e-9, rel
    sc.close(); short.close()
