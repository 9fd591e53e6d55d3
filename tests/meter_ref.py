"""The C restatement of the loudness meter's arithmetic contract (tests/cpp/meter_ref.c), built with gcc and called through ctypes; a
float64 model of the same contract in plain Python loops (every fma evaluated exactly in rational arithmetic and rounded once); and the
signals shared by tests/test_meter_cpu.py and tests/test_gpu_meter.py."""
import ctypes as C
import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "meter_ref.c"
BINS, RING = 1000, 30
# include/fmdemod.h fmd_meter_status
STATUS_DTYPE = np.dtype([("frames", "<u8"), ("subblocks", "<u8"), ("energy_ring", "<f8", (RING,)), ("peak_call", "<f4", (2,)),
                         ("peak_hold", "<f4", (2,)), ("below_gate", "<u4"), ("nonfinite", "<u4")])
assert STATUS_DTYPE.itemsize == 280


class Design(C.Structure):
    _fields_ = [("pre_b", C.c_double * 3), ("pre_a", C.c_double * 3), ("rlb_b", C.c_double * 3), ("rlb_a", C.c_double * 3),
                ("nsb", C.c_int), ("edge", C.c_double * (BINS + 1)), ("centre", C.c_double * BINS)]


class _Status(C.Structure):
    _fields_ = [("frames", C.c_ulonglong), ("subblocks", C.c_ulonglong), ("energy_ring", C.c_double * RING), ("peak_call", C.c_float * 2),
                ("peak_hold", C.c_float * 2), ("below_gate", C.c_uint), ("nonfinite", C.c_uint)]


class _Chan(C.Structure):
    _fields_ = [("st", _Status)] + [(k, C.c_double * 2) for k in ("s1", "s2", "t1", "t2", "acc")] + [("hist", C.c_uint * BINS)]


class Channel:
    """one station of the restatement: process(x [n, 2] float32) as often as wanted, then status() / hist()"""

    def __init__(self, ref, fs: int):
        self.lib, self.d = ref.lib, ref.design(fs)
        self.c = _Chan()
        self.lib.meter_ref_reset(C.byref(self.c))

    def process(self, x):
        x = np.ascontiguousarray(x, np.float32)
        assert x.ndim == 2 and x.shape[1] == 2
        self.lib.meter_ref_process(C.byref(self.d), C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0])
        return self

    def reset(self):
        self.lib.meter_ref_reset(C.byref(self.c))

    def reset_peaks(self):
        self.lib.meter_ref_reset_peaks(C.byref(self.c))

    def status(self) -> np.ndarray:
        """a [1] STATUS_DTYPE record array (a copy)"""
        return np.frombuffer(bytes(self.c.st), STATUS_DTYPE).copy()

    def hist(self) -> np.ndarray:
        return np.frombuffer(bytes(self.c.hist), np.uint32).copy()

    def integrated(self) -> float:
        return self.lib.meter_ref_integrated(self.c.hist, C.byref(self.d))

    def momentary(self):
        out = C.c_double(0.0)
        rc = self.lib.meter_ref_momentary(C.byref(self.c.st), C.byref(out))
        return out.value if rc == 0 else None

    def short_term(self):
        out = C.c_double(0.0)
        rc = self.lib.meter_ref_short_term(C.byref(self.c.st), C.byref(out))
        return out.value if rc == 0 else None


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def design(self, fs: int) -> Design:
        d = Design()
        if self.lib.meter_ref_design(int(fs), C.byref(d)) != 0:
            raise ValueError(f"fs {fs}")
        return d

    def channel(self, fs: int) -> Channel:
        return Channel(self, fs)

    def run(self, fs: int, x) -> Channel:
        """a fresh station fed x [n, 2] in one piece"""
        return Channel(self, fs).process(x)


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libmeter_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.meter_ref_design.argtypes = [C.c_int, C.POINTER(Design)]
    lib.meter_ref_reset.argtypes = [C.POINTER(_Chan)]
    lib.meter_ref_reset.restype = None
    lib.meter_ref_reset_peaks.argtypes = [C.POINTER(_Chan)]
    lib.meter_ref_reset_peaks.restype = None
    lib.meter_ref_process.argtypes = [C.POINTER(Design), C.POINTER(_Chan), C.c_void_p, C.c_longlong]
    lib.meter_ref_process.restype = None
    lib.meter_ref_lufs.argtypes = [C.c_double]
    lib.meter_ref_lufs.restype = C.c_double
    lib.meter_ref_momentary.argtypes = [C.POINTER(_Status), C.POINTER(C.c_double)]
    lib.meter_ref_short_term.argtypes = [C.POINTER(_Status), C.POINTER(C.c_double)]
    lib.meter_ref_integrated.argtypes = [C.c_void_p, C.POINTER(Design)]
    lib.meter_ref_integrated.restype = C.c_double
    return Ref(lib)


def bits(a) -> np.ndarray:
    """an array's bytes (status records, float64 and float32 arrays compare bit for bit, NaNs and signed zeros included)"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


# ---- the float64 model ----------------------------------------------------------------------------------------------------------

def _fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (finite operands): exact in rationals, and float() of a Fraction rounds to nearest even"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def model_design(fs: int) -> dict:
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Vh = math.pow(10.0, 3.999843853973347 / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    Q = 0.7071752369554196
    a0 = 1.0 + K / Q + K * K
    pre_b = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    pre_a = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    rlb_a = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return {"pre_b": pre_b, "pre_a": pre_a, "rlb_b": [1.0, -2.0, 1.0], "rlb_a": rlb_a, "nsb": fs // 10,
            "edge": [math.pow(10.0, ((-70.0 + 0.1 * j) + 0.691) / 10.0) for j in range(BINS + 1)],
            "centre": [math.pow(10.0, (((-70.0 + 0.1 * j) + 0.05) + 0.691) / 10.0) for j in range(BINS)]}


def model_run(fs: int, x: np.ndarray) -> dict:
    """a fresh station fed x [n, 2] float32 (finite samples), frame after frame: {"energies": [G] float64, "hist": [1000] uint32,
    "peak": [2] float32, "below_gate": int}"""
    d = model_design(fs)
    pb0, pb1, pb2 = d["pre_b"]
    _, pa1, pa2 = d["pre_a"]
    rb0, rb1, rb2 = d["rlb_b"]
    _, ra1, ra2 = d["rlb_a"]
    nsb, edge = d["nsb"], d["edge"]
    s1, s2, t1, t2, acc = [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]
    peak = [np.float32(0.0), np.float32(0.0)]
    energies, hist, below = [], np.zeros(BINS, np.uint32), 0
    for f in range(x.shape[0]):
        for r in range(2):
            v = float(x[f, r])
            o1 = _fma(pb0, v, s1[r])
            s1[r] = _fma(-pa1, o1, _fma(pb1, v, s2[r]))
            s2[r] = _fma(-pa2, o1, pb2 * v)
            o2 = _fma(rb0, o1, t1[r])
            t1[r] = _fma(-ra1, o2, _fma(rb1, o1, t2[r]))
            t2[r] = _fma(-ra2, o2, rb2 * o1)
            acc[r] = _fma(o2, o2, acc[r])
            peak[r] = max(peak[r], np.abs(x[f, r]))
        if (f + 1) % nsb == 0:
            energies.append((acc[0] + acc[1]) / float(nsb))
            acc = [0.0, 0.0]
            g = len(energies) - 1
            if g >= 3:
                B = (((energies[g - 3] + energies[g - 2]) + energies[g - 1]) + energies[g]) * 0.25
                if B < edge[0]:
                    below += 1
                else:
                    hist[max(j for j in range(BINS) if edge[j] <= B)] += 1
    return {"energies": np.array(energies, np.float64), "hist": hist, "peak": np.array(peak, np.float32), "below_gate": below}


# ---- signals --------------------------------------------------------------------------------------------------------------------

def stepped_noise(C_: int, n: int, seed: int = 5) -> np.ndarray:
    """[C, n, 2] float32 noise with a 60 dB level step in the middle, a different level per station (L and R differ by 3 dB)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C_, n, 2))
    for c in range(C_):
        x[c] *= 0.25 * 10.0 ** (-c / 2.0)
        x[c, n // 2:] *= 1e-3 if c % 2 == 0 else 1.0
        x[c, :n // 2] *= 1.0 if c % 2 == 0 else 1e-3
    x[:, :, 1] *= 10.0 ** (-3.0 / 20.0)
    return x.astype(np.float32)


def sine(fs: int, seconds: float, hz: float, dbfs_l, dbfs_r) -> np.ndarray:
    """[n, 2] float32 sine; a level of None is silence on that rail"""
    t = np.arange(int(round(fs * seconds)), dtype=np.float64) / fs
    s = np.sin(2.0 * np.pi * hz * t)
    x = np.zeros((t.size, 2), np.float64)
    for r, lv in enumerate((dbfs_l, dbfs_r)):
        if lv is not None:
            x[:, r] = 10.0 ** (lv / 20.0) * s
    return x.astype(np.float32)
