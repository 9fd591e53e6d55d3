"""The C restatement of the loudness meter's true peak and loudness range (tests/cpp/meter_r128_ref.c, which compiles tests/cpp/meter_ref.c
in), built with gcc and called through ctypes; an independent model of the interpolator's design and of fmd_meter_range in Python and
numpy; and the signals shared by tests/test_meter_r128_cpu.py and tests/test_gpu_meter_r128.py."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np

import meter_ref
from meter_ref import BINS, Design, _Chan

SRC = Path(__file__).resolve().parent / "cpp" / "meter_r128_ref.c"
TRUE_PEAK, RANGE = 1, 2
TAPS, HIST = 12, 11
# include/fmdemod.h fmd_meter_r128_status
R128_DTYPE = np.dtype([("tp_call", "<f4", (2,)), ("tp_hold", "<f4", (2,)), ("st_below", "<u4"), ("st_nonfinite", "<u4")])
assert R128_DTYPE.itemsize == 24


class TpDesign(C.Structure):
    _fields_ = [("L", C.c_int), ("taps_per_phase", C.c_int), ("taps", (C.c_float * TAPS) * 3)]


class _R128Status(C.Structure):
    _fields_ = [("tp_call", C.c_float * 2), ("tp_hold", C.c_float * 2), ("st_below", C.c_uint), ("st_nonfinite", C.c_uint)]


class _R128Chan(C.Structure):
    _fields_ = [("base", _Chan), ("st", _R128Status), ("hist", (C.c_float * HIST) * 2), ("range_hist", C.c_uint * BINS)]


class Channel:
    """one station of the restatement: process(x [n, 2] float32) as often as wanted, then status() / hist() / r128() / range_hist()"""

    def __init__(self, ref, fs: int, features: int):
        self.lib, self.d, self.tp, self.features = ref.lib, ref.design(fs), ref.tp_design(fs), int(features)
        self.c = _R128Chan()
        self.lib.meter_r128_reset(C.byref(self.c))

    def process(self, x):
        x = np.ascontiguousarray(x, np.float32)
        assert x.ndim == 2 and x.shape[1] == 2
        self.lib.meter_r128_process(C.byref(self.d), C.byref(self.tp), self.features, C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0])
        return self

    def reset(self):
        self.lib.meter_r128_reset(C.byref(self.c))

    def reset_peaks(self):
        self.lib.meter_r128_reset_peaks(C.byref(self.c))

    def status(self) -> np.ndarray:
        return np.frombuffer(bytes(self.c.base.st), meter_ref.STATUS_DTYPE).copy()

    def hist(self) -> np.ndarray:
        return np.frombuffer(bytes(self.c.base.hist), np.uint32).copy()

    def r128(self) -> np.ndarray:
        """a [1] R128_DTYPE record array (a copy)"""
        return np.frombuffer(bytes(self.c.st), R128_DTYPE).copy()

    def range_hist(self) -> np.ndarray:
        return np.frombuffer(bytes(self.c.range_hist), np.uint32).copy()

    def history(self) -> np.ndarray:
        """[2, 11] float32: the interpolator's carried frames per rail, oldest first"""
        return np.frombuffer(bytes(self.c.hist), np.float32).reshape(2, HIST).copy()

    def loudness_range(self):
        """(lra, low, high), or None where no bin survives the gates"""
        return Ref(self.lib).range(self.range_hist(), self.d)


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def design(self, fs: int) -> Design:
        d = Design()
        if self.lib.meter_ref_design(int(fs), C.byref(d)) != 0:
            raise ValueError(f"fs {fs}")
        return d

    def tp_design(self, fs: int) -> TpDesign:
        d = TpDesign()
        if self.lib.meter_r128_tp_design(int(fs), C.byref(d)) != 0:
            raise ValueError(f"fs {fs}")
        return d

    def channel(self, fs: int, features: int = TRUE_PEAK | RANGE) -> Channel:
        return Channel(self, fs, features)

    def run(self, fs: int, x, features: int = TRUE_PEAK | RANGE) -> Channel:
        """a fresh station fed x [n, 2] in one piece"""
        return Channel(self, fs, features).process(x)

    def range(self, hist, d: Design):
        h = np.ascontiguousarray(hist, np.uint32)
        out = [C.c_double(0.0) for _ in range(3)]
        rc = self.lib.meter_r128_range(h.ctypes.data_as(C.c_void_p), C.byref(d), *[C.byref(v) for v in out])
        return tuple(v.value for v in out) if rc == 0 else None


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libmeter_r128_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.meter_ref_design.argtypes = [C.c_int, C.POINTER(Design)]
    lib.meter_r128_tp_design.argtypes = [C.c_int, C.POINTER(TpDesign)]
    lib.meter_r128_reset.argtypes = [C.POINTER(_R128Chan)]
    lib.meter_r128_reset.restype = None
    lib.meter_r128_reset_peaks.argtypes = [C.POINTER(_R128Chan)]
    lib.meter_r128_reset_peaks.restype = None
    lib.meter_r128_process.argtypes = [C.POINTER(Design), C.POINTER(TpDesign), C.c_uint, C.POINTER(_R128Chan), C.c_void_p, C.c_longlong]
    lib.meter_r128_process.restype = None
    lib.meter_r128_dbtp.argtypes = [C.c_float]
    lib.meter_r128_dbtp.restype = C.c_double
    lib.meter_r128_range.argtypes = [C.c_void_p, C.POINTER(Design), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return Ref(lib)


def taps_array(d) -> np.ndarray:
    """[3, 12] float32 of a TpDesign-shaped ctypes structure (the restatement's or the library's)"""
    return np.array([[d.taps[p][k] for k in range(TAPS)] for p in range(3)], np.float32)


# ---- the independent model ------------------------------------------------------------------------------------------------------

def _i0(x: float) -> float:
    s = term = 1.0
    for k in range(1, 64):
        term *= (x / (2.0 * k)) * (x / (2.0 * k))
        s += term
        if term < 1e-18 * s:
            break
    return s


def model_tp_design(fs: int):
    """(L, [3, 12] float32): the Kaiser-windowed sinc of the contract, written from its formula (libm's sin and sqrt through `math`)"""
    L = 4 if fs < 88200 else 2 if fs < 176400 else 1
    N = L * TAPS
    c = float(N // 2)
    h = []
    for i in range(N):
        x = (i - c) / L
        r = (i - c) / c
        s = 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)
        h.append(s * _i0(5.0 * math.sqrt(1.0 - r * r)) / _i0(5.0))
    taps = np.zeros((3, TAPS), np.float32)
    for p in range(1, L):
        g = h[p::L]
        total = 0.0
        for v in g:
            total += v
        taps[p - 1] = np.array([v / total for v in g], np.float64).astype(np.float32)
    return L, taps


def model_range(hist, centre):
    """fmd_meter_range by sorting the values instead of walking the bins: (lra, low, high), or None"""
    hist = np.asarray(hist, np.uint32).astype(np.uint64)
    centre = np.asarray(centre, np.float64)
    n0 = int(hist.sum())
    if n0 == 0:
        return None
    s = 0.0
    for j in range(BINS):
        s += float(hist[j]) * centre[j]
    keep = centre >= 0.01 * (s / float(n0))
    kept = np.where(keep, hist, 0)
    n = int(kept.sum())
    if n == 0:
        return None
    cum = np.cumsum(kept)                                   # cum[j] values lie in bins <= j: rank r is in the first bin with cum > r
    r10, r95 = (int(math.floor(q * (n - 1) + 0.5)) for q in (0.10, 0.95))
    j10, j95 = (int(np.searchsorted(cum, r, side="right")) for r in (r10, r95))
    return (j95 - j10) / 10.0, -70.0 + 0.1 * j10 + 0.05, -70.0 + 0.1 * j95 + 0.05


# ---- signals --------------------------------------------------------------------------------------------------------------------

# EBU Tech 3341's true-peak cases in spirit: (amplitude, fs divisor, phase in degrees, expected dBTP)
TP_SINES = [(0.5, 4, 0.0, -6.0206), (0.5, 4, 45.0, -6.0206), (0.5, 6, 60.0, -6.0206), (0.5, 8, 67.5, -6.0206), (1.41, 4, 45.0, 2.9844)]
TP_TOL = (-0.4, 0.2)           # EBU Tech 3341: reading - expected within +0.2 / -0.4 dB


def tp_sine(n: int, amp: float, div: int, phase_deg: float, fade: int = 96) -> np.ndarray:
    """[n, 2] float32: amp * sin(2 pi i / div + phase) on both rails, faded in over `fade` frames by a raised cosine.  The known answer
    "true peak = amplitude" is a property of the sinusoid; a sine switched on at a non-zero phase is a sinusoid plus a step, and the
    step's band-limited overshoot is real true peak (it reads up to 0.67 dB high at fs/8 and 67.5 degrees with fade = 0)."""
    i = np.arange(n, dtype=np.float64)
    s = amp * np.sin(2.0 * np.pi * i / div + np.deg2rad(phase_deg))
    s[:fade] *= 0.5 - 0.5 * np.cos(np.pi * np.arange(fade) / fade)
    return np.stack([s, s], axis=1).astype(np.float32)


def level_steps(fs: int, levels_lufs, seconds: float = 20.0) -> np.ndarray:
    """[n, 2] float32: a stereo 1 kHz sine, `seconds` at each level (a stereo sine of amplitude a reads 20 log10(a) LUFS at 1 kHz)"""
    parts = []
    t0 = 0
    for lv in levels_lufs:
        n = int(round(fs * seconds))
        t = (np.arange(n, dtype=np.float64) + t0) / fs
        s = 10.0 ** (lv / 20.0) * np.sin(2.0 * np.pi * 1000.0 * t)
        parts.append(np.stack([s, s], axis=1))
        t0 += n
    return np.concatenate(parts).astype(np.float32)
