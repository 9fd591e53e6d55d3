"""The C restatement of the carrier squelch's arithmetic contract (tests/cpp/squelch_ref.c), built with gcc and called through ctypes;
a float64 model of the same contract in plain Python loops (every fma evaluated exactly and rounded once); and the signals shared by
tests/test_squelch_cpu.py and tests/test_gpu_squelch.py."""
import ctypes as C
import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "squelch_ref.c"
NP, RING = 256, 20
AUTO, FORCE_OPEN, FORCE_CLOSED = 0, 1, 2
# include/fmdemod.h fmd_squelch_status
STATUS_DTYPE = np.dtype([("samples", "<u8"), ("intervals", "<u8"), ("intervals_open", "<u8"), ("ring_s2", "<f8", (RING,)), ("ring_s4", "<f8", (RING,)),
                         ("last_peak", "<f4"), ("hold_peak", "<f4"), ("run", "<u4"), ("transitions", "<u4"), ("nonfinite", "<u4"),
                         ("open", "u1"), ("mode", "u1"), ("reserved", "u1", (2,))])
assert STATUS_DTYPE.itemsize == 368


class Params(C.Structure):
    _fields_ = [("open_db", C.c_double), ("close_db", C.c_double), ("min_level_db", C.c_double), ("open_intervals", C.c_int),
                ("close_intervals", C.c_int), ("mode", C.c_int)]


class _Status(C.Structure):
    _fields_ = [("samples", C.c_ulonglong), ("intervals", C.c_ulonglong), ("intervals_open", C.c_ulonglong), ("ring_s2", C.c_double * RING),
                ("ring_s4", C.c_double * RING), ("last_peak", C.c_float), ("hold_peak", C.c_float), ("run", C.c_uint), ("transitions", C.c_uint),
                ("nonfinite", C.c_uint), ("open", C.c_ubyte), ("mode", C.c_ubyte), ("reserved", C.c_ubyte * 2)]


class _Chan(C.Structure):
    _fields_ = [("st", _Status), ("prm", Params), ("M", C.c_int), ("c_open", C.c_double), ("c_close", C.c_double), ("min_s2", C.c_double),
                ("pk", C.c_float), ("p", (C.c_double * NP) * 2), ("mask", C.c_ubyte)]


assert C.sizeof(_Status) == 368 and C.sizeof(Params) == 40


class Channel:
    """one station of the restatement: process(x [n, 2] float32 or uint8) as often as wanted, then status(), mask and the read-outs"""

    def __init__(self, ref, fs: int):
        self.lib, self.fs = ref.lib, int(fs)
        self.c = _Chan()
        if self.lib.squelch_ref_create(C.byref(self.c), int(fs)) != 0:
            raise ValueError(f"fs {fs}")

    def process(self, x):
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype in (np.float32, np.uint8)
        fn = self.lib.squelch_ref_process_cf32 if x.dtype == np.float32 else self.lib.squelch_ref_process_u8
        fn(C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0])
        return self

    def set_params(self, **fields) -> int:
        """0, or -1 where the restatement rejects the values (nothing changes then)"""
        p = Params.from_buffer_copy(bytes(self.c.prm))
        for k, v in fields.items():
            setattr(p, k, v)
        return self.lib.squelch_ref_set_params(C.byref(self.c), C.byref(p))

    def reset(self):
        self.lib.squelch_ref_reset(C.byref(self.c))

    def reset_peaks(self):
        self.lib.squelch_ref_reset_peaks(C.byref(self.c))

    @property
    def mask(self) -> int:
        """the station's mask byte as of the last process call (0xAA before the first)"""
        return int(self.c.mask)

    def status(self) -> np.ndarray:
        """a [1] STATUS_DTYPE record array (a copy)"""
        return np.frombuffer(bytes(self.c.st), STATUS_DTYPE).copy()

    def _read(self, fn, *args):
        out = C.c_double(0.0)
        rc = getattr(self.lib, fn)(C.byref(self.c.st), self.fs, *args, C.byref(out))
        return out.value if rc == 0 else None

    def level_db(self):
        return self._read("squelch_ref_level_db")

    def cnr_db(self, window: int = 1):
        return self._read("squelch_ref_cnr_db", C.c_int(window))

    def powers(self, window: int = 1):
        return ref_powers(self.lib, self.status(), self.fs, window)[1:]


def ref_powers(lib, record, fs: int, window: int):
    """(rc, carrier, noise) of one STATUS_DTYPE record"""
    r = np.ascontiguousarray(record, STATUS_DTYPE).reshape(-1)
    a, b = C.c_double(0.0), C.c_double(0.0)
    rc = lib.squelch_ref_powers(r.ctypes.data_as(C.c_void_p), int(fs), int(window), C.byref(a), C.byref(b))
    return rc, a.value, b.value


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def channel(self, fs: int) -> Channel:
        return Channel(self, fs)

    def run(self, fs: int, x, **params) -> Channel:
        """a fresh station (with these parameters) fed x [n, 2] in one piece"""
        ch = Channel(self, fs)
        if params:
            assert ch.set_params(**params) == 0
        return ch.process(x)

    def threshold(self, db: float) -> float:
        return self.lib.squelch_ref_threshold(float(db))

    def default_params(self) -> Params:
        p = Params()
        self.lib.squelch_ref_default_params(C.byref(p))
        return p

    def readout(self, fn: str, record, fs: int, *args):
        """(rc, value) of squelch_ref_level_db / squelch_ref_cnr_db over one STATUS_DTYPE record"""
        r = np.ascontiguousarray(record, STATUS_DTYPE).reshape(-1)
        out = C.c_double(0.0)
        rc = getattr(self.lib, fn)(r.ctypes.data_as(C.c_void_p), int(fs), *[C.c_int(a) for a in args], C.byref(out))
        return rc, out.value


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libsquelch_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.squelch_ref_create.argtypes = [C.POINTER(_Chan), C.c_int]
    lib.squelch_ref_default_params.argtypes = [C.POINTER(Params)]
    lib.squelch_ref_default_params.restype = None
    lib.squelch_ref_threshold.argtypes = [C.c_double]
    lib.squelch_ref_threshold.restype = C.c_double
    lib.squelch_ref_set_params.argtypes = [C.POINTER(_Chan), C.POINTER(Params)]
    for fn in ("squelch_ref_reset", "squelch_ref_reset_peaks"):
        getattr(lib, fn).argtypes = [C.POINTER(_Chan)]
        getattr(lib, fn).restype = None
    for fn in ("squelch_ref_process_cf32", "squelch_ref_process_u8"):
        getattr(lib, fn).argtypes = [C.POINTER(_Chan), C.c_void_p, C.c_longlong]
        getattr(lib, fn).restype = None
    lib.squelch_ref_level_db.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    lib.squelch_ref_cnr_db.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.squelch_ref_powers.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return Ref(lib)


def bits(a) -> np.ndarray:
    """an array's bytes (status records, float64 and float32 arrays compare bit for bit, NaNs and signed zeros included)"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


# ---- the float64 model ----------------------------------------------------------------------------------------------------------

def _fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (finite operands): exact in rationals, and float() of a Fraction rounds to nearest even"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def model_threshold(db: float) -> float:
    k = math.pow(10.0, db / 10.0)
    return (k * k) / ((1.0 + k) * (1.0 + k))


def model_cnr_db(s2, s4, M: int):
    """cnr_db over the intervals given (oldest first): the read-out's definition"""
    e2 = e4 = 0.0
    for a, b in zip(s2, s4):
        e2, e4 = e2 + a, e4 + b
    N = float(M) * float(len(s2))
    d = _fma(-N, e4, 2.0 * e2 * e2)
    if d <= 0.0:
        return -math.inf
    c = math.sqrt(d) / N
    nz = e2 / N - c
    return math.inf if nz <= 0.0 else 10.0 * math.log10(c / nz)


def model_run(fs: int, x: np.ndarray, open_db=10.0, close_db=7.0, min_level_db=-math.inf, open_intervals=2, close_intervals=10) -> dict:
    """a fresh station fed x [n, 2] float32 (finite samples), sample after sample.  {"intervals": [per completed interval a dict of S2, S4,
    pk, good_open, good_close, open, run], "hold_peak", "pk" (the open interval's), "part": the open interval's [2][256] partials,
    "transitions", "intervals_open"}"""
    M = fs // 20
    c_open, c_close = model_threshold(open_db), model_threshold(close_db)
    min_s2 = 0.0 if min_level_db == -math.inf else math.pow(10.0, min_level_db / 10.0) * float(M)
    part = [[0.0] * NP, [0.0] * NP]
    pk = hold = 0.0
    is_open, run, transitions, n_open = False, 0, 0, 0
    out = {"intervals": []}
    xi, xq = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)
    pw = xi * xi + xq * xq                  # fma(I, I, Q * Q): both products are exact in double, so the sum is rounded once either way
    mx = np.maximum(np.abs(x[:, 0]), np.abs(x[:, 1]))
    for n in range(x.shape[0]):
        r = n % M
        j = r % NP
        p = float(pw[n])
        part[0][j] = part[0][j] + p
        part[1][j] = _fma(p, p, part[1][j])
        m = float(mx[n])
        pk, hold = max(pk, m), max(hold, m)
        if r + 1 == M:
            S = []
            for q in part:
                w = NP // 2
                while w >= 1:
                    for jj in range(w):
                        q[jj] += q[jj + w]
                    w //= 2
                S.append(q[0])
            S2, S4 = S
            a = S2 * S2
            d = _fma(-float(M), S4, 2.0 * a)
            finite = math.isfinite(S2) and math.isfinite(S4)
            good_open = finite and S2 >= min_s2 and d > c_open * a
            good_close = finite and S2 >= min_s2 and d > c_close * a
            if not is_open:
                run = run + 1 if good_open else 0
                if run >= open_intervals:
                    is_open, run, transitions = True, 0, transitions + 1
            else:
                run = 0 if good_close else run + 1
                if run >= close_intervals:
                    is_open, run, transitions = False, 0, transitions + 1
            n_open += int(is_open)
            out["intervals"].append({"S2": S2, "S4": S4, "pk": pk, "good_open": good_open, "good_close": good_close, "open": is_open, "run": run,
                                     "cnr_db": model_cnr_db([S2], [S4], M)})
            part = [[0.0] * NP, [0.0] * NP]
            pk = 0.0
    out.update(hold_peak=hold, pk=pk, part=part, transitions=transitions, intervals_open=n_open)
    return out


# ---- signals --------------------------------------------------------------------------------------------------------------------

# the gate sequence of tests/test_squelch_cpu.py and tests/test_gpu_squelch.py: (CNR in dB or None for an absent carrier, intervals)
GATE_PATTERN = ((None, 3), (20.0, 1), (None, 1), (20.0, 4), (8.5, 3), (None, 2), (20.0, 1), (None, 3), (8.5, 3), (20.0, 2))
GATE_TAIL = 777                        # samples of an open interval behind the pattern (at 20 dB)
GATE_PARAMS = dict(open_db=10.0, close_db=7.0, open_intervals=2, close_intervals=3)
# the mask after each interval of the pattern (open_intervals = 2, close_intervals = 3)
GATE_MASK = [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1]
GATE_SEED = 5


def gate_levels(lead: int = 0, total: int | None = None) -> list:
    """the pattern's CNR per interval behind `lead` intervals without a carrier, continued at 20 dB up to `total` intervals"""
    lv = [None] * lead + [db for db, k in GATE_PATTERN for _ in range(k)]
    return lv + [20.0] * (0 if total is None else total - len(lv))


def expected_masks(levels, open_db=10.0, close_db=7.0, open_intervals=2, close_intervals=3) -> list:
    """the gate after every interval for intervals that read their nominal CNR: (masks, transitions)"""
    is_open, run, tr, out = False, 0, 0, []
    for lv in levels:
        if not is_open:
            run = run + 1 if lv is not None and lv > open_db else 0
            if run >= open_intervals:
                is_open, run, tr = True, 0, tr + 1
        else:
            run = 0 if lv is not None and lv > close_db else run + 1
            if run >= close_intervals:
                is_open, run, tr = False, 0, tr + 1
        out.append(int(is_open))
    return out, tr


def gate_signal(fs: int, amplitude: float, seed: int = GATE_SEED, lead: int = 0, total: int | None = None) -> np.ndarray:
    """[n, 2] float64, n = intervals * M + GATE_TAIL: a noise-FM carrier of this amplitude that is present or absent per interval of
    gate_levels(lead, total), in complex Gaussian noise whose power per interval puts the carrier at that interval's CNR (the 8.5 dB
    noise where the carrier is absent)"""
    M = fs // 20
    lv = gate_levels(lead, total)
    n = len(lv) * M + GATE_TAIL
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n + 64)
    v = np.convolve(v, np.hanning(9) / np.hanning(9).sum(), mode="same")[32:32 + n]
    ph = 2.0 * np.pi * np.cumsum(50000.0 * v / (3.5 * v.std()) + 2300.0) / fs
    per = np.repeat(np.array([np.nan if a is None else a for a in lv + [20.0]]), M)[:n]
    on = ~np.isnan(per)
    sigma2 = amplitude ** 2 / 10.0 ** (np.where(on, per, 8.5) / 10.0)
    z = np.where(on, amplitude, 0.0) * np.exp(1j * ph) + np.sqrt(0.5 * sigma2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.stack([z.real, z.imag], axis=1)


def to_u8(x: np.ndarray) -> np.ndarray:
    """a receiver's bytes of x, which is in LSB already: round(127 + x), clipped"""
    return np.clip(np.rint(np.asarray(x, np.float64) + 127.0), 0, 255).astype(np.uint8)


def from_u8(b: np.ndarray) -> np.ndarray:
    """the floats the squelch sees for those bytes: (float)v - 127"""
    return b.astype(np.float32) - np.float32(127.0)


def interval_cnr_db(x: np.ndarray, M: int) -> list:
    """the read-out's definition in vectorised float64 (plain sums, not the contract's order): cnr_db of every whole interval of x [n, 2]"""
    p = np.asarray(x[:, 0], np.float64) ** 2 + np.asarray(x[:, 1], np.float64) ** 2
    k = p.size // M
    s2 = p[:k * M].reshape(k, M).sum(1)
    s4 = (p[:k * M] ** 2).reshape(k, M).sum(1)
    return [model_cnr_db([a], [b], M) for a, b in zip(s2, s4)]
