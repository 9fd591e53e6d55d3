"""DC offset and IQ imbalance corrector on the GPU (fmd_iqcorr_*): the moments against exact integer sums and, for cf32, bit for bit against
the C restatement of their summation order (tests/cpp/iqcorr_ref.c); bit identity over splits into calls, streams and formats; the applied
correction bit for bit against the restatement; image rejection on an impaired two-station capture; and the band scanner's detections with
and without the correction."""
import numpy as np
import pytest

import iqcorr_ref
from conftest import bits_equal, describe_diff
from scan_ref import ref_detect, ref_psd

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 777
RANGES = {"u8": (0, 256), "s8": (-128, 128), "s16": (-32768, 32768)}
CORR = (0.37, -1.21, 0.031, -0.047)          # a non-trivial correction (values that are not fp32 numbers: rounded on the way in)


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    return p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return iqcorr_ref.build(tmp_path_factory.mktemp("iqcorr_ref"))


@pytest.fixture(scope="module")
def two_stations():
    """(clean capture x, impaired capture z as complex64) of tests 5 and 6"""
    x = iqcorr_ref.two_station_capture()
    return x, iqcorr_ref.impair(x, 1.05, 3.0).astype(np.complex64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pairs(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1).astype(np.float32))


def _raw(rng, fmt, n):
    lo, hi = RANGES[fmt]
    return rng.integers(lo, hi, size=(n, 2)).astype(iqcorr_ref.FORMATS[fmt][1])


def _int_moments(raw, fmt):
    v = raw.astype(np.int64) - (127 if fmt == "u8" else 0)
    i, q = v[:, 0], v[:, 1]
    return [float(w) for w in (len(v), i.sum(), q.sum(), (i * i).sum(), (q * q).sum(), (i * q).sum())]


def _cf32_capture(rng, n):
    """60 dB of dynamic range plus a DC term, as test_gpu_scan.py's _capture"""
    t = np.arange(n, dtype=np.float64)
    x = 1e-2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 0.05
    for f, a in ((0.1234, 10.0), (-0.3071, 3.0), (0.41, 0.01)):
        x = x + a * np.exp(2j * np.pi * ((f * t) % 1.0))
    return _pairs(x)


def _mbits(m):
    return np.array(m, np.float64).view(np.uint64)


@pytest.mark.parametrize("fmt", ["u8", "s8", "s16"])
def test_integer_moments_are_exact(pkg, fmt):
    """random captures and the extremes (every sample at the format's lowest and highest value), n = 3 chunks + 777: the fp64 sums are the
    int64 sums.  Also a capture of more than 1024 chunks (s8): the fold kernel's second LDS tile."""
    rng = np.random.default_rng(5)
    lo, hi = RANGES[fmt]
    dt = iqcorr_ref.FORMATS[fmt][1]
    cases = [_raw(rng, fmt, N), np.full((N, 2), lo, dt), np.full((N, 2), hi - 1, dt)]
    if fmt == "s8":
        cases.append(_raw(rng, fmt, 1025 * 4096 + 5))
    for k, raw in enumerate(cases):
        co = pkg.IqCorrector(max_input_samples=len(raw))
        if k % 2:
            co.measure(_dev(raw))
        else:
            co.process(_dev(raw))
        got = list(co.moments())
        assert got == _int_moments(raw, fmt), (fmt, k)
        co.close()


def test_cf32_moments_are_bit_identical_to_the_restatement(pkg, ref):
    rng = np.random.default_rng(6)
    for n in (N, 9 * 4096, 300):
        x = _cf32_capture(rng, n)
        co = pkg.IqCorrector(max_input_samples=n)
        co.measure(_dev(x))
        got, want = co.moments(), ref.moments(x)
        assert np.array_equal(_mbits(got), _mbits(want)), (n, list(got), list(want))
        co.close()


def test_ragged_calls_streams_and_formats_are_bit_identical(pkg, ref):
    """one call == ragged calls cut at 1, 2, around 256, around a chunk's end, inside and across chunks, alternating over two streams and
    over two formats (the s16 samples as they are, and the same values as cf32); moments() between two cuts reports the capture so far
    and disturbs nothing"""
    import torch
    rng = np.random.default_rng(8)
    raw = _raw(rng, "s16", N)
    conv = raw.astype(np.float32)
    rt, ct = _dev(raw), _dev(conv)
    one = pkg.IqCorrector(max_input_samples=N)
    one.correction = CORR
    y_one = one.process(rt).cpu().numpy()
    m_one = one.moments()
    cuts = [0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 8191, 2 * 4096 + 9, 3 * 4096 + 9, 3 * 4096 + 300, N]
    rag = pkg.IqCorrector(max_input_samples=N)
    rag.correction = CORR
    out = torch.zeros((N, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        src = rt if k % 3 != 1 else ct
        rag.process(src[a:b], out=out[a:b], stream=streams[k & 1])
        if b in (257, 4097, 3 * 4096 + 9):
            mid = rag.moments()
            assert np.array_equal(_mbits(mid), _mbits(ref.moments(conv[:b]))), b
    m_rag = rag.moments()
    torch.cuda.synchronize()
    assert np.array_equal(_mbits(m_rag), _mbits(m_one))
    assert list(m_one) == _int_moments(raw, "s16")
    assert bits_equal(out.cpu().numpy(), y_one), describe_diff(out.cpu().numpy(), y_one)
    assert bits_equal(y_one, ref.apply(conv, np.array(one.correction, np.float32)))
    # the same over a cf32 capture, whose sums round: one call, the restatement and the ragged calls agree to the bit
    x = _cf32_capture(rng, N)
    xt = _dev(x)
    a1 = pkg.IqCorrector(max_input_samples=N)
    a1.measure(xt)
    a2 = pkg.IqCorrector(max_input_samples=N)
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        a2.measure(xt[a:b], stream=streams[k & 1])
        if b == 8191:
            a2.moments()
    want = ref.moments(x)
    assert np.array_equal(_mbits(a1.moments()), _mbits(want)) and np.array_equal(_mbits(a2.moments()), _mbits(want))
    torch.cuda.synchronize()
    for c in (one, rag, a1, a2):
        c.close()


@pytest.mark.parametrize("fmt", ["cf32", "u8", "s8", "s16"])
def test_apply_is_bit_identical_to_the_restatement(pkg, ref, fmt):
    """a non-trivial correction; d_in and d_out starting 0, 1 and 3 samples into an aligned array (every 16-byte phase of every format);
    20 chunks + 333 samples (several workgroups); in place for cf32; measure-only leaves the same moments; the identity correction is
    the conversion"""
    import torch
    rng = np.random.default_rng(12)
    n = 20 * 4096 + 333
    raw = _cf32_capture(rng, n + 3) if fmt == "cf32" else _raw(rng, fmt, n + 3)
    big = _dev(raw)
    corr32 = None
    for off in (0, 1, 3):
        src, x = big[off:off + n], ref.convert(raw[off:off + n], fmt)
        co = pkg.IqCorrector(max_input_samples=n)
        co.correction = CORR
        corr32 = np.array(co.correction, np.float32)
        assert bits_equal(corr32, np.array(CORR, np.float32))
        outbuf = torch.full((n + 4, 2), -7.0, dtype=torch.float32, device="cuda")
        y = co.process(src, out=outbuf[off:off + n]).cpu().numpy()
        want = ref.apply(x, corr32)
        assert bits_equal(y, want), (fmt, off, describe_diff(y, want))
        guard = outbuf.cpu().numpy()
        assert (guard[:off] == -7.0).all() and (guard[off + n:] == -7.0).all()          # nothing written outside [n_in][2]
        m_write = co.moments()
        assert np.array_equal(_mbits(m_write), _mbits(ref.moments(x)))
        co.reset_moments()
        assert co.process(src, out=False) is None
        assert np.array_equal(_mbits(co.moments()), _mbits(m_write))
        assert co.correction == pkg.IqCorrection(*[float(v) for v in corr32])         # reset_moments keeps the correction
        co.close()
    x = ref.convert(raw[:n], fmt)
    ident = pkg.IqCorrector(max_input_samples=n)
    assert ident.correction == pkg.IqCorrection(0.0, 0.0, 0.0, 0.0)
    assert np.array_equal(ident.process(big[:n]).cpu().numpy(), x)
    # 16-byte loads with 8-byte stores, and the other way round
    shifted = torch.empty((n + 1, 2), dtype=torch.float32, device="cuda")
    assert np.array_equal(ident.process(big[:n], out=shifted[1:]).cpu().numpy(), x)
    assert np.array_equal(ident.process(big[1:n + 1], out=shifted[:n]).cpu().numpy(), ref.convert(raw[1:n + 1], fmt))
    if fmt == "cf32":
        ident.correction = CORR
        for off in (0, 1):
            buf = big[off:off + n].clone() if off == 0 else big.clone()[off:off + n]
            got = ident.process(buf, out=buf)
            assert got.data_ptr() == buf.data_ptr()
            assert bits_equal(got.cpu().numpy(), ref.apply(ref.convert(raw[off:off + n], fmt), corr32))
    ident.close()


def test_image_rejection(pkg, two_stations):
    """Two FM stations (noise-like programme, 60 kHz peak deviation) at +400 kHz (amplitude 1.0) and -200 kHz (0.3) of 2.048 MSa/s,
    n = 131 849, noise sigma 1e-3 per component, impaired with g = 1.05, phi = 3 degrees, d = 0.02 - 0.01j.  The residual image is the
    amplitude ratio of a least-squares fit of the output onto {x, conj(x), 1}.  Condition: the float64 restatement leaves the image at or
    below -60 dB.  Bar: the GPU result is at most 3 dB worse than the restatement on the same capture.
    Float64 model on this capture: -28.9 dB before, -117 dB after.  The GPU's figure is printed; none has been recorded yet."""
    x, z = two_stations
    zp = _pairs(z)
    before = iqcorr_ref.image_db(z, x)
    z64 = z.astype(np.complex128)
    dc, w = iqcorr_ref.solve64(iqcorr_ref.moments64(z64))
    model = iqcorr_ref.image_db(iqcorr_ref.apply64(z64, dc, w), x)
    assert model <= -60.0, model
    co = pkg.IqCorrector(max_input_samples=len(z))
    zt = _dev(zp)
    co.measure(zt)
    c = co.calibrate()
    assert co.correction == c and co.moments().n == len(z)
    y = co.process(zt).cpu().numpy()
    gpu = iqcorr_ref.image_db(y[:, 0].astype(np.float64) + 1j * y[:, 1], x)
    print(f"image: {before:.1f} dB before, {model:.1f} dB float64 restatement, {gpu:.1f} dB GPU; w = {c.w_re:+.6f} {c.w_im:+.6f}j, "
          f"dc = {c.dc_i:+.6f} {c.dc_q:+.6f}j")
    assert before > -32.0
    assert gpu <= model + 3.0, (gpu, model)
    assert abs(complex(c.w_re, c.w_im) - w) < 1e-7 and abs(complex(c.dc_i, c.dc_q) - dc) < 1e-7
    co.close()


def test_scanner_sees_ghosts_without_the_correction_and_none_with_it(pkg, two_stations):
    """The same capture through BandScanner with its defaults.  Uncorrected: the two stations, their images at -400 kHz and +200 kHz and
    the DC carrier at 0.  Corrected: exactly {-200 kHz, +400 kHz}.  The float64 definition (tests/scan_ref.py) gives the same two sets,
    checked here on the same data."""
    x, z = two_stations
    ghosts, clean = [-400e3, -200e3, 0.0, 200e3, 400e3], [-200e3, 400e3]
    fs = iqcorr_ref.FS_TWO
    zt = _dev(_pairs(z))
    co = pkg.IqCorrector(max_input_samples=len(z))
    co.measure(zt)
    co.calibrate()
    yt = co.process(zt)
    found = []
    for t in (zt, yt):
        sc = pkg.BandScanner(fs, max_input_samples=len(z))
        sc.process(t)
        found.append(sc.stations())
        a = t.cpu().numpy().astype(np.float64)
        want = ref_detect(ref_psd(a[:, 0] + 1j * a[:, 1], sc.nfft, fs)[0], fs)
        assert [r[0] for r in want] == list(found[-1]["offset_hz"])
        sc.close()
    print("uncorrected:", [(float(s["offset_hz"]), round(float(s["snr_db"]), 1)) for s in found[0]])
    print("corrected:  ", [(float(s["offset_hz"]), round(float(s["snr_db"]), 1)) for s in found[1]])
    assert list(found[0]["offset_hz"]) == ghosts
    assert list(found[1]["offset_hz"]) == clean
    co.close()


def test_arguments(pkg):
    import torch
    rng = np.random.default_rng(2)
    raw = _raw(rng, "s16", 5000)
    rt = _dev(raw)
    co = pkg.IqCorrector(max_input_samples=4999)
    co.correction = CORR
    co.process(rt[:4999])
    before = co.moments()
    out = torch.full((5000, 2), -7.0, dtype=torch.float32, device="cuda")
    for bad in (rt[:0], rt):                                   # n_in = 0 and n_in > max_input_samples
        with pytest.raises(pkg.FmdError) as e:
            co.process(bad, out=out[:bad.shape[0]])
        assert e.value.status == -1                            # FMD_ERR_ARG
    assert (out.cpu().numpy() == -7.0).all()
    assert np.array_equal(_mbits(co.moments()), _mbits(before)) and before.n == 4999
    for bad in ((np.nan, 0, 0, 0), (0, np.inf, 0, 0), (0, 0, -np.inf, 0), (0, 0, 0, np.nan)):
        with pytest.raises(pkg.FmdError) as e:
            co.correction = bad
        assert e.value.status == -1
    assert bits_equal(np.array(co.correction, np.float32), np.array(CORR, np.float32))
    with pytest.raises(ValueError):
        co.process(rt[:100], out=out[:99])
    co.reset()
    assert co.moments() == pkg.IqMoments(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert co.correction == pkg.IqCorrection(0.0, 0.0, 0.0, 0.0)
    with pytest.raises(pkg.FmdError):                          # nothing measured: no correction to solve
        co.calibrate()
    co.process(rt[:100])                                       # after a reset the count starts again at sample 0
    assert list(co.moments()) == _int_moments(raw[:100], "s16")
    co.close()
