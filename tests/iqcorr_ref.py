"""The C restatement of the IQ corrector's arithmetic contract (tests/cpp/iqcorr_ref.c), built with gcc and called through ctypes, a
float64 model of the correction, and the impaired two-station capture shared by tests/test_iqcorr_cpu.py and tests/test_gpu_iqcorr.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "iqcorr_ref.c"
FORMATS = {"cf32": (0, np.float32), "u8": (1, np.uint8), "s8": (2, np.int8), "s16": (3, np.int16)}
D_OFFSET = 0.02 - 0.01j


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def convert(self, raw: np.ndarray, fmt: str) -> np.ndarray:
        """raw [n, 2] of the format's type -> [n, 2] float32"""
        code, dt = FORMATS[fmt]
        raw = np.ascontiguousarray(raw, dt)
        out = np.empty(raw.shape, np.float32)
        self.lib.iqcorr_ref_convert(raw.ctypes.data_as(C.c_void_p), code, raw.shape[0], out.ctypes.data_as(C.c_void_p))
        return out

    def moments(self, x: np.ndarray) -> np.ndarray:
        """x [n, 2] float32 (converted samples) -> float64 [6]: n, sum i, sum q, sum i^2, sum q^2, sum i q in the fixed order"""
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty(6, np.float64)
        self.lib.iqcorr_ref_moments(x.ctypes.data_as(C.c_void_p), x.shape[0], out.ctypes.data_as(C.c_void_p))
        return out

    def solve(self, m):
        """six moments -> float32 [4] (dc_i, dc_q, w_re, w_im), or None where the library returns FMD_ERR_ARG"""
        m = np.ascontiguousarray(m, np.float64)
        out = np.zeros(4, np.float32)
        rc = self.lib.iqcorr_ref_solve(m.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out if rc == 0 else None

    def apply(self, x: np.ndarray, corr) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        corr = np.ascontiguousarray(corr, np.float32)
        y = np.empty_like(x)
        self.lib.iqcorr_ref_apply(x.ctypes.data_as(C.c_void_p), x.shape[0], corr.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p))
        return y


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libiqcorr_ref.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.iqcorr_ref_convert.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p]
    lib.iqcorr_ref_convert.restype = None
    lib.iqcorr_ref_moments.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
    lib.iqcorr_ref_moments.restype = None
    lib.iqcorr_ref_solve.argtypes = [C.c_void_p, C.c_void_p]
    lib.iqcorr_ref_solve.restype = C.c_int
    lib.iqcorr_ref_apply.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.iqcorr_ref_apply.restype = None
    return Ref(lib)


def impair(x: np.ndarray, g: float, phi_deg: float, d: complex = D_OFFSET) -> np.ndarray:
    """a x + b conj(x) + d with a = (1 + g e^{-j phi}) / 2, b = (1 - g e^{j phi}) / 2: a receiver whose Q arm has gain g and phase error phi"""
    a, b = imbalance(g, phi_deg)
    return a * x + b * np.conj(x) + d


def imbalance(g: float, phi_deg: float) -> tuple[complex, complex]:
    phi = np.deg2rad(phi_deg)
    return (1 + g * np.exp(-1j * phi)) / 2, (1 - g * np.exp(1j * phi)) / 2


def moments64(z: np.ndarray) -> np.ndarray:
    """the six moments of a complex128 array by plain float64 sums (no fixed order: a model, not the contract)"""
    i, q = z.real, z.imag
    return np.array([z.size, i.sum(), q.sum(), (i * i).sum(), (q * q).sum(), (i * q).sum()], np.float64)


def solve64(m) -> tuple[complex, complex]:
    """the solve step in float64 numpy, unrounded: (dc, w)"""
    n, si, sq, sii, sqq, siq = (float(v) for v in m)
    mi, mq = si / n, sq / n
    vii, vqq, viq = sii / n - mi * mi, sqq / n - mq * mq, siq / n - mi * mq
    p, c = vii + vqq, complex(vii - vqq, 2 * viq)
    s = np.sqrt(max(0.0, p * p - abs(c) ** 2))
    return complex(mi, mq), (-c / (p + s) if p + s > 0 else 0j)


def apply64(z: np.ndarray, dc: complex, w: complex) -> np.ndarray:
    u = z - dc
    return u + w * np.conj(u)


def image_db(y: np.ndarray, x: np.ndarray) -> float:
    """least-squares fit of y onto {x, conj(x), 1}: the image's amplitude over the signal's, in dB"""
    y = np.asarray(y, np.complex128)
    x = np.asarray(x, np.complex128)
    A = np.stack([x, np.conj(x), np.ones_like(x)], axis=1)
    coef = np.linalg.lstsq(A, y, rcond=None)[0]
    return float(20 * np.log10(abs(coef[1]) / abs(coef[0])))


FS_TWO = 2_048_000.0
N_TWO = 131_849


def _fm_station(rng, n: int, fs: float, offset_hz: float, dev_hz: float = 60e3) -> np.ndarray:
    """unit-modulus FM with a noise-like programme (white noise low-passed to about 15 kHz, peak-normalised), peak deviation dev_hz"""
    m = rng.standard_normal(n + 256)
    k = np.hanning(137)
    m = np.convolve(m, k / k.sum(), mode="same")[128:128 + n]
    m /= np.max(np.abs(m))
    phase = 2 * np.pi * np.cumsum(dev_hz * m + offset_hz) / fs
    return np.exp(1j * phase)


def two_station_capture(seed: int = 21) -> np.ndarray:
    """the clean capture of the image-rejection tests (complex128): stations at +400 kHz (amplitude 1.0) and -200 kHz (0.3) of
    2.048 MSa/s, n = 131 849, complex noise of sigma 1e-3 per component"""
    rng = np.random.default_rng(seed)
    x = 1.0 * _fm_station(rng, N_TWO, FS_TWO, 400e3) + 0.3 * _fm_station(rng, N_TWO, FS_TWO, -200e3)
    return x + 1e-3 * (rng.standard_normal(N_TWO) + 1j * rng.standard_normal(N_TWO))
