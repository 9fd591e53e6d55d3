"""Float64 restatement of the band scanner (include/fmdemod.h, "Band scan"): the averaged periodogram and the detection rules, and a
synthesiser of wideband captures with FM stations planted on a raster over a white noise floor.  Shared by tests/test_scan_cpu.py and
tests/test_gpu_scan.py."""
import math

import numpy as np

import synth

FS_STATION = 256_000.0
DEFAULTS = dict(raster_hz=100e3, raster_origin_hz=0.0, channel_bw_hz=100e3, min_snr_db=10.0, usable_fraction=0.8, noise_quantile=0.1,
                min_spacing_hz=150e3)


def hann(nfft: int) -> np.ndarray:
    """the periodic Hann window as the library stores it (fp32), in float64"""
    n = np.arange(nfft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / nfft)).astype(np.float32).astype(np.float64)


def ref_psd(x: np.ndarray, nfft: int, fs_in: float, chunk: int = 256) -> tuple[np.ndarray, int]:
    """(PSD [nfft] fft-shifted, frame count): frames [f H, f H + N), H = N / 2, no padding; S = sum_f |FFT(w x_f)|^2 in float64"""
    x = np.asarray(x, np.complex128)
    hop = nfft // 2
    frames = (x.size - nfft) // hop + 1 if x.size >= nfft else 0
    w = hann(nfft)
    s = np.zeros(nfft)
    for f0 in range(0, frames, chunk):
        idx = (np.arange(f0, min(frames, f0 + chunk)) * hop)[:, None] + np.arange(nfft)[None, :]
        s += (np.abs(np.fft.fft(x[idx] * w, axis=1)) ** 2).sum(axis=0)
    if frames == 0:
        return np.zeros(nfft), 0
    return np.fft.fftshift(s) / (frames * fs_in * float(np.sum(w * w))), frames


def ref_detect(psd: np.ndarray, fs_in: float, **params) -> list[tuple[float, float, float]]:
    """the detection rules: [(offset_hz, power_db, snr_db)] ascending by offset"""
    p = dict(DEFAULTS, **params)
    psd = np.asarray(psd, np.float64)
    n = psd.size
    h = n // 2
    delta = fs_in / n
    lim = p["usable_fraction"] * fs_in / 2
    f = (np.arange(n) - h) * delta
    usable = np.sort(psd[np.abs(f) <= lim])
    nu = usable[int(math.floor(p["noise_quantile"] * (usable.size - 1)))]
    cands = []
    raster, origin, half = p["raster_hz"], p["raster_origin_hz"], p["channel_bw_hz"] / 2
    j = math.floor((-lim - origin) / raster) - 1
    while origin + j * raster <= lim + raster:
        fc = origin + j * raster
        j += 1
        if not abs(fc) + half <= lim:
            continue
        lo, hi = max(0, math.ceil((fc - half) / delta) + h), min(n - 1, math.floor((fc + half) / delta) + h)   # clipped to the N bins
        if hi < lo:
            continue
        pc = delta * float(np.sum(psd[lo:hi + 1]))
        if not pc > 0:
            continue
        snr = 10 * math.log10(pc / (nu * delta * (hi - lo + 1))) if nu > 0 else math.inf
        if snr >= p["min_snr_db"]:
            cands.append((fc, pc, snr))
    cands.sort(key=lambda c: (-c[1], c[0]))
    acc = []
    for c in cands:
        if all(abs(a[0] - c[0]) >= p["min_spacing_hz"] for a in acc):
            acc.append(c)
    return [(fc, 10 * math.log10(pc), snr) for fc, pc, snr in sorted(acc)]


def station_amplitude(snr_db: float, fs_in: float, noise_power: float = 1.0, bw_hz: float = 100e3) -> float:
    """amplitude of a unit-modulus FM station whose power is snr_db above the floor's power in bw_hz"""
    return math.sqrt(10 ** (snr_db / 10) * noise_power * bw_hz / fs_in)


def plant_station(args) -> np.ndarray:
    """one station of a capture at fs_in: synth.fm_capture (no noise of its own) at 256 kSa/s, resampled up, scaled and shifted to its
    offset.  args = (n, fs_in, offset_hz, snr_db, channel, seed); usable as a worker-pool task."""
    from scipy.signal import resample_poly
    n, fs_in, offset_hz, snr_db, channel, seed = args
    up = int(round(fs_in / FS_STATION))
    assert up * FS_STATION == fs_in
    st = synth.fm_capture(-(-n // up) + 64, fs=FS_STATION, seed=seed, channel=channel, noise_sigma=0.0)["iq"]
    y = resample_poly(st, up, 1)[:n]
    t = np.arange(n, dtype=np.float64)
    return station_amplitude(snr_db, fs_in) * y * np.exp(2j * np.pi * ((offset_hz / fs_in * t) % 1.0))


def noise_floor(n: int, seed: int) -> np.ndarray:
    """white complex Gaussian of unit power"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * math.sqrt(0.5)


def plant(n: int, fs_in: float, stations, seed: int = 1) -> np.ndarray:
    """stations = [(offset_hz, snr_db, channel)]: the capture (complex128) over a unit-power floor"""
    x = noise_floor(n, seed)
    for off, snr, ch in stations:
        x = x + plant_station((n, fs_in, off, snr, ch, 500 + ch))
    return x
