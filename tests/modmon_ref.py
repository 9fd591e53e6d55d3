"""The C restatement of the FM modulation monitor's arithmetic contract (tests/cpp/modmon_ref.c), built with gcc and called through
ctypes; a float64 model of the same contract in plain Python loops (every fma and fmaf evaluated exactly and rounded once); and the
signals shared by tests/test_modmon_cpu.py and tests/test_gpu_modmon.py."""
import ctypes as C
import ctypes.util
import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "modmon_ref.c"
TAPS, NP, BINS, RING, MAXP = 33, 64, 300, 60, 384
# include/fmdemod.h fmd_modmon_status
STATUS_DTYPE = np.dtype([("samples", "<u8"), ("intervals", "<u8"), ("seconds", "<u8"), ("last_hi", "<f4"), ("last_lo", "<f4"),
                         ("hold_hi", "<f4"), ("hold_lo", "<f4"), ("last_s1", "<f8"), ("last_s2", "<f8"), ("last_sc", "<f8"),
                         ("last_ss", "<f8"), ("sec_e", "<f8", (RING,)), ("sec_f", "<f8", (RING,)), ("sec_q", "<f8", (RING,)),
                         ("sec_n", "<u4", (RING,)), ("open_e", "<f8"), ("open_f", "<f8"), ("open_q", "<f8"), ("open_n", "<u4"),
                         ("over", "<u4"), ("nonfinite", "<u4"), ("reserved", "<u4")])
assert STATUS_DTYPE.itemsize == 1792


class Design(C.Structure):
    _fields_ = [("fs", C.c_int), ("M", C.c_int), ("P", C.c_int), ("reserved", C.c_int), ("hz_per_rad", C.c_double), ("pilot_gain", C.c_double),
                ("h", C.c_float * TAPS), ("reserved_f", C.c_float), ("pilot_cos", C.c_double * MAXP), ("pilot_sin", C.c_double * MAXP),
                ("edge", C.c_double * (BINS + 1))]


class _Status(C.Structure):
    _fields_ = [("samples", C.c_ulonglong), ("intervals", C.c_ulonglong), ("seconds", C.c_ulonglong), ("last_hi", C.c_float),
                ("last_lo", C.c_float), ("hold_hi", C.c_float), ("hold_lo", C.c_float), ("last_s1", C.c_double), ("last_s2", C.c_double),
                ("last_sc", C.c_double), ("last_ss", C.c_double), ("sec_e", C.c_double * RING), ("sec_f", C.c_double * RING),
                ("sec_q", C.c_double * RING), ("sec_n", C.c_uint * RING), ("open_e", C.c_double), ("open_f", C.c_double),
                ("open_q", C.c_double), ("open_n", C.c_uint), ("over", C.c_uint), ("nonfinite", C.c_uint), ("reserved", C.c_uint)]


class _Chan(C.Structure):
    _fields_ = [("st", _Status), ("theta", C.c_float), ("d", C.c_float * TAPS), ("hi", C.c_float), ("lo", C.c_float),
                ("p", (C.c_double * NP) * 4), ("hist", C.c_uint * BINS)]


assert C.sizeof(_Status) == 1792


class Channel:
    """one station of the restatement: process(x [n, 2] float32 or uint8) as often as wanted, then status() / hist() and the read-outs"""

    def __init__(self, ref, fs: int):
        self.lib, self.d = ref.lib, ref.design(fs)
        self.c = _Chan()
        self.lib.modmon_ref_reset(C.byref(self.c))

    def process(self, x):
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype in (np.float32, np.uint8)
        fn = self.lib.modmon_ref_process_cf32 if x.dtype == np.float32 else self.lib.modmon_ref_process_u8
        fn(C.byref(self.d), C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0])
        return self

    def reset(self):
        self.lib.modmon_ref_reset(C.byref(self.c))

    def reset_peaks(self):
        self.lib.modmon_ref_reset_peaks(C.byref(self.c))

    def status(self) -> np.ndarray:
        """a [1] STATUS_DTYPE record array (a copy)"""
        return np.frombuffer(bytes(self.c.st), STATUS_DTYPE).copy()

    def hist(self) -> np.ndarray:
        return np.frombuffer(bytes(self.c.hist), np.uint32).copy()

    def _read(self, fn, *args):
        out = C.c_double(0.0)
        rc = getattr(self.lib, fn)(C.byref(self.c.st), C.byref(self.d), *args, C.byref(out))
        return out.value if rc == 0 else None

    def deviation_hz(self):
        return self._read("modmon_ref_deviation_hz")

    def offset_hz(self):
        return self._read("modmon_ref_offset_hz")

    def pilot_hz(self):
        return self._read("modmon_ref_pilot_hz")

    def mpx_power_dbr(self, window_s: int):
        return self._read("modmon_ref_mpx_power_dbr", C.c_int(window_s))


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def design(self, fs: int) -> Design:
        d = Design()
        if self.lib.modmon_ref_design(int(fs), C.byref(d)) != 0:
            raise ValueError(f"fs {fs}")
        return d

    def channel(self, fs: int) -> Channel:
        return Channel(self, fs)

    def run(self, fs: int, x) -> Channel:
        """a fresh station fed x [n, 2] in one piece"""
        return Channel(self, fs).process(x)

    def exceedance(self, hist, over: int, limit_hz: int):
        """(rc, fraction, count)"""
        h = np.ascontiguousarray(hist, np.uint32)
        frac, cnt = C.c_double(0.0), C.c_ulonglong(0)
        rc = self.lib.modmon_ref_exceedance(h.ctypes.data_as(C.c_void_p), int(over), int(limit_hz), C.byref(frac), C.byref(cnt))
        return rc, frac.value, cnt.value

    def percentile(self, hist, over: int, q: float):
        """(rc, hz)"""
        h = np.ascontiguousarray(hist, np.uint32)
        out = C.c_double(0.0)
        rc = self.lib.modmon_ref_percentile(h.ctypes.data_as(C.c_void_p), int(over), float(q), C.byref(out))
        return rc, out.value


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libmodmon_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.modmon_ref_design.argtypes = [C.c_int, C.POINTER(Design)]
    for fn in ("modmon_ref_reset", "modmon_ref_reset_peaks"):
        getattr(lib, fn).argtypes = [C.POINTER(_Chan)]
        getattr(lib, fn).restype = None
    for fn in ("modmon_ref_process_cf32", "modmon_ref_process_u8"):
        getattr(lib, fn).argtypes = [C.POINTER(Design), C.POINTER(_Chan), C.c_void_p, C.c_longlong]
        getattr(lib, fn).restype = None
    for fn in ("modmon_ref_deviation_hz", "modmon_ref_offset_hz", "modmon_ref_pilot_hz"):
        getattr(lib, fn).argtypes = [C.POINTER(_Status), C.POINTER(Design), C.POINTER(C.c_double)]
    lib.modmon_ref_mpx_power_dbr.argtypes = [C.POINTER(_Status), C.POINTER(Design), C.c_int, C.POINTER(C.c_double)]
    lib.modmon_ref_exceedance.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]
    lib.modmon_ref_percentile.argtypes = [C.c_void_p, C.c_uint, C.c_double, C.POINTER(C.c_double)]
    return Ref(lib)


def bits(a) -> np.ndarray:
    """an array's bytes (status records, float64 and float32 arrays compare bit for bit, NaNs and signed zeros included)"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


# ---- the float64 model ----------------------------------------------------------------------------------------------------------

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.argtypes = [C.c_float, C.c_float]
_libm.atan2f.restype = C.c_float


def _fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (finite operands): exact in rationals, and float() of a Fraction rounds to nearest even"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _f32(x: float) -> float:
    return float(np.float32(x))


def _fmaf(a: float, b: float, c: float) -> float:
    """a * b + c of three float32 values (held in Python floats), rounded once to float32.  The product is exact in double and fsum
    rounds the exact sum once to double; rounding that to float32 is a second rounding only where the double is exactly half way
    between two float32 values, and only there the exact rational decides."""
    r = math.fsum((a * b, c))
    f = _f32(r)
    if f == r:
        return f
    g = float(np.nextafter(np.float32(f), np.float32(math.copysign(math.inf, r - f))))
    if r != 0.5 * (f + g):
        return f
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    return f if abs(exact - Fraction(f)) < abs(exact - Fraction(g)) else g if exact != Fraction(r) else f


def _i0(x: float) -> float:
    s, term = 1.0, 1.0
    for k in range(1, 64):
        term *= (x / (2.0 * k)) * (x / (2.0 * k))
        s += term
        if term < 1e-18 * s:
            break
    return s


def _sinc(x: float) -> float:
    return 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)


def model_design(fs: int) -> dict:
    M, P = fs // 20, fs // math.gcd(fs, 19000)
    w, i0b = 2.0 * 76000.0 / float(fs), _i0(5.0)
    g, total = [], 0.0
    for i in range(TAPS):
        x, r = w * float(i - 16), float(i - 16) / 16.0
        g.append(((w * _sinc(x)) * _i0(5.0 * math.sqrt(1.0 - r * r))) / i0b)
        total += g[-1]
    h = [_f32(v / total) for v in g]
    ang = [(2.0 * math.pi * float((19000 * k) % fs)) / float(fs) for k in range(P)]
    re = im = 0.0
    for i in range(TAPS):
        a = (2.0 * math.pi * float(19000 * i)) / float(fs)
        re += h[i] * math.cos(a)
        im += h[i] * math.sin(a)
    return {"fs": fs, "M": M, "P": P, "hz_per_rad": float(fs) / (2.0 * math.pi), "h": h, "pilot_cos": [math.cos(a) for a in ang],
            "pilot_sin": [math.sin(a) for a in ang], "pilot_gain": math.sqrt(re * re + im * im) * _sinc(19000.0 / float(fs)),
            "edge": [500.0 * j for j in range(BINS + 1)]}


def model_run(fs: int, x: np.ndarray) -> dict:
    """a fresh station fed x [n, 2] float32 (finite samples), sample after sample.  {"intervals": [per completed interval a dict of hi, lo
    (float32 values), S1, S2, Sc, Ss, D], "hist": [300] uint32, "over": int, "hold_hi", "hold_lo", "open": (e, f, q, n),
    "seconds": [(e, f, q, n)]}"""
    d = model_design(fs)
    h, M, P, hz, pc, ps = d["h"], d["M"], d["P"], d["hz_per_rad"], d["pilot_cos"], d["pilot_sin"]
    pi32 = np.float32(math.pi)
    two_pi32 = np.float32(2.0) * pi32
    dl = [0.0] * TAPS
    theta_prev = np.float32(0.0)
    hi, lo, hold_hi, hold_lo = -math.inf, math.inf, -math.inf, math.inf
    part = [[0.0] * NP for _ in range(4)]
    out = {"intervals": [], "hist": np.zeros(BINS, np.uint32), "over": 0, "seconds": []}
    oe = of = oq = 0.0
    on = 0
    for n in range(x.shape[0]):
        theta = np.float32(_libm.atan2f(float(x[n, 1]), float(x[n, 0])))
        if n == 0:
            dn = np.float32(0.0)
        else:
            dn = theta - theta_prev
            if dn >= pi32:
                dn = dn - two_pi32
            elif dn <= -pi32:
                dn = dn + two_pi32
        theta_prev = theta
        dl = [float(dn)] + dl[:-1]
        y = 0.0
        for t in range(TAPS):
            y = _fmaf(h[t], dl[t], y)
        hi, lo, hold_hi, hold_lo = max(hi, y), min(lo, y), max(hold_hi, y), min(hold_lo, y)
        fd = y * hz
        r = n % M
        j, k = r % NP, n % P
        part[0][j] = part[0][j] + fd
        part[1][j] = _fma(fd, fd, part[1][j])
        part[2][j] = _fma(fd, pc[k], part[2][j])
        part[3][j] = _fma(fd, ps[k], part[3][j])
        if r + 1 == M:
            S = []
            for p in part:
                w = NP // 2
                while w >= 1:
                    for jj in range(w):
                        p[jj] += p[jj + w]
                    w //= 2
                S.append(p[0])
            D = 0.5 * (hi - lo) * hz
            out["intervals"].append({"hi": hi, "lo": lo, "S1": S[0], "S2": S[1], "Sc": S[2], "Ss": S[3], "D": D})
            if D >= d["edge"][BINS]:
                out["over"] += 1
            else:
                out["hist"][max(jj for jj in range(BINS) if d["edge"][jj] <= D)] += 1
            oe, of, oq, on = oe + S[1], of + S[0], oq + _fma(S[2], S[2], S[3] * S[3]), on + 1
            if len(out["intervals"]) % 20 == 0:
                out["seconds"].append((oe, of, oq, on))
                oe = of = oq = 0.0
                on = 0
            hi, lo = -math.inf, math.inf
            part = [[0.0] * NP for _ in range(4)]
    out.update(hold_hi=hold_hi, hold_lo=hold_lo, open=(oe, of, oq, on))
    return out


# ---- signals --------------------------------------------------------------------------------------------------------------------

def noise_fm(C_: int, n: int, fs: int, seed: int = 11) -> np.ndarray:
    """[C, n, 2] float32: carriers frequency-modulated by band-limited noise, station c with peak deviation near 25 (c + 1) kHz, a carrier
    (1 + c) * 1.7 kHz off (alternating sign) and its own amplitude"""
    rng = np.random.default_rng(seed)
    out = np.empty((C_, n, 2), np.float32)
    for c in range(C_):
        v = rng.standard_normal(n + 64)
        v = np.convolve(v, np.hanning(9) / np.hanning(9).sum(), mode="same")[32:32 + n]   # roughly 0 ... 50 kHz at 192 kSa/s
        f = 25000.0 * (c + 1) * v / (3.5 * v.std()) + (1 + c) * 1700.0 * (-1.0) ** c
        ph = 2.0 * np.pi * np.cumsum(f) / fs
        a = 0.9 / (1 + c)
        out[c, :, 0] = a * np.cos(ph)
        out[c, :, 1] = a * np.sin(ph)
    return out


def to_u8(x: np.ndarray) -> np.ndarray:
    """a receiver's bytes of x (full scale 1.0 -> +-120 around 127)"""
    return np.clip(np.rint(np.asarray(x, np.float64) * 120.0 + 127.0), 0, 255).astype(np.uint8)


def from_u8(b: np.ndarray) -> np.ndarray:
    """the floats the monitor sees for those bytes: (float)v - 127"""
    return b.astype(np.float32) - np.float32(127.0)


def tones(fs: int, n: int, tone_hz: float = 400.0, tone_dev: float = 19000.0, pilot_dev: float = 6750.0, offset_hz: float = 1500.0,
          pilot_phase: float = 0.4) -> np.ndarray:
    """[n, 2] float32: a carrier offset_hz off, modulated by a tone_hz sinusoid of +-tone_dev and a 19 kHz pilot of +-pilot_dev.  The phase
    is the closed-form integral of the instantaneous frequency, not a cumulative sum: the discriminator then sees what a real transmitter
    sends, with its own sinc(f / fs) response to each line"""
    t = np.arange(n, dtype=np.float64) / fs
    ph = 2.0 * np.pi * offset_hz * t - (tone_dev / tone_hz) * np.cos(2.0 * np.pi * tone_hz * t) \
        - (pilot_dev / 19000.0) * np.cos(2.0 * np.pi * 19000.0 * t + pilot_phase)
    return np.stack([np.cos(ph), np.sin(ph)], axis=1).astype(np.float32)
