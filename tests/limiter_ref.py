"""The C restatement of the look-ahead peak limiter's arithmetic contract (tests/cpp/limiter_ref.c), built with gcc and called through
ctypes; a numpy restatement written the other way (vectorised, the release through its closed form, the windows through
sliding_window_view); and the signals shared by tests/test_limiter_cpu.py and tests/test_gpu_limiter.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SRC = Path(__file__).resolve().parent / "cpp" / "limiter_ref.c"
ONE = 1 << 30
MAX_D = 255
FS = 32000
# include/fmdemod.h fmd_limiter_status
STATUS_DTYPE = np.dtype([("frames", "<u8"), ("limited", "<u8"), ("clamped", "<u8", (2,)), ("nonfinite", "<u8"), ("min_gain", "<f4"), ("gain", "<f4"),
                         ("eq", "<u4"), ("reserved", "u1", (12,))])
assert STATUS_DTYPE.itemsize == 64 and STATUS_DTYPE.fields["clamped"][1] == 16 and STATUS_DTYPE.fields["nonfinite"][1] == 32
assert STATUS_DTYPE.fields["min_gain"][1] == 40 and STATUS_DTYPE.fields["gain"][1] == 44 and STATUS_DTYPE.fields["eq"][1] == 48

# (D, step) of the GPU comparison, and the milliseconds at FS that design to them: D = llround(ms * 32), step = llround(2^30 / (ms * 32))
DS = (0, 1, 47, 255)
STEPS = (1, 6711, ONE)
LOOKAHEAD_MS = {0: 0.0, 1: 1.0 / 32.0, 47: 47.0 / 32.0, 255: 255.0 / 32.0}
RELEASE_MS = {1: float(ONE) / 32.0, 6711: 5000.0, ONE: 0.0}
CEILING_DB = -1.0
GAINS = (0.5, 1.7, 4.0)


class _Status(C.Structure):
    _fields_ = [("frames", C.c_ulonglong), ("limited", C.c_ulonglong), ("clamped", C.c_ulonglong * 2), ("nonfinite", C.c_ulonglong), ("min_gain", C.c_float),
                ("gain", C.c_float), ("eq", C.c_uint), ("reserved", C.c_ubyte * 12)]


class _Chan(C.Structure):
    _fields_ = [("st", _Status), ("D", C.c_int), ("step", C.c_uint), ("T", C.c_float), ("pos", C.c_ulonglong), ("rq", C.c_uint * 256), ("eq", C.c_uint * 256),
                ("u", C.c_float * 512)]


assert C.sizeof(_Status) == 64


def ceiling(ceiling_db: float = CEILING_DB) -> np.float32:
    """T as the design states it"""
    return np.float32(10.0 ** (ceiling_db / 20.0))


class Channel:
    """one station of the restatement: process(x [n, 2] float32) -> (y [n, 2] float32, the call's smallest g); flush(); status()"""

    def __init__(self, lib, D: int, step: int, T, gain: float = 1.0):
        self.lib = lib
        self.c = _Chan()
        if lib.limiter_ref_create(C.byref(self.c), int(D), int(step), C.c_float(float(T))) != 0:
            raise ValueError(f"D {D}, step {step}, T {T}")
        self.D = int(D)
        self.set_gain(gain)

    def set_gain(self, gain: float):
        self.lib.limiter_ref_set_gain(C.byref(self.c), C.c_float(float(gain)))

    def process(self, x) -> tuple:
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype == np.float32
        y = np.zeros_like(x)
        g = self.lib.limiter_ref_process(C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0], y.ctypes.data_as(C.c_void_p))
        return y, np.float32(g)

    def flush(self) -> np.ndarray:
        y = np.zeros((self.D, 2), np.float32)
        assert self.lib.limiter_ref_flush(C.byref(self.c), y.ctypes.data_as(C.c_void_p)) == self.D
        return y

    def reset(self):
        self.lib.limiter_ref_reset(C.byref(self.c))

    def status(self) -> np.ndarray:
        """a [1] STATUS_DTYPE record array (a copy)"""
        return np.frombuffer(bytes(self.c.st), STATUS_DTYPE).copy()

    def set_frames(self, frames: int):
        """the frame count alone, for a station that has been running for long"""
        self.c.st.frames = int(frames)

    @property
    def eq(self) -> int:
        return int(self.c.st.eq)


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def channel(self, D: int, step: int, T, gain: float = 1.0) -> Channel:
        return Channel(self.lib, D, step, T, gain)

    def rq(self, ul: float, ur: float, T) -> int:
        return int(self.lib.limiter_ref_rq(C.c_float(float(ul)), C.c_float(float(ur)), C.c_float(float(T))))


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "liblimiter_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.limiter_ref_create.argtypes = [C.POINTER(_Chan), C.c_int, C.c_uint, C.c_float]
    lib.limiter_ref_reset.argtypes = [C.POINTER(_Chan)]
    lib.limiter_ref_reset.restype = None
    lib.limiter_ref_set_gain.argtypes = [C.POINTER(_Chan), C.c_float]
    lib.limiter_ref_set_gain.restype = None
    lib.limiter_ref_rq.argtypes = [C.c_float, C.c_float, C.c_float]
    lib.limiter_ref_rq.restype = C.c_uint
    lib.limiter_ref_process.argtypes = [C.POINTER(_Chan), C.c_void_p, C.c_longlong, C.c_void_p]
    lib.limiter_ref_process.restype = C.c_float
    lib.limiter_ref_flush.argtypes = [C.POINTER(_Chan), C.c_void_p]
    return Ref(lib)


def bits(a) -> np.ndarray:
    """an array's bytes"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------------

def gained(x, gain) -> tuple:
    """(u [n, 2] float32 with the non-finite products as +0, their number)"""
    with np.errstate(all="ignore"):
        u = np.asarray(x, np.float32) * np.float32(gain)
    bad = ~np.isfinite(u)
    return np.where(bad, np.float32(0.0), u).astype(np.float32), int(bad.sum())


def numpy_limiter(x, gain, D: int, step: int, T, flush: bool = False) -> dict:
    """a whole stream from a reset, at once: y (with the flush's D frames behind it where asked), rq, mq, eq, S, g and the counters"""
    T = np.float32(T)
    W = D + 1
    u, nonfinite = gained(x, gain)
    frames = u.shape[0]
    if flush:
        u = np.concatenate([u, np.zeros((D, 2), np.float32)])
    n = u.shape[0]
    p = np.max(np.abs(u), axis=1)
    over = p > T
    with np.errstate(all="ignore"):
        q = (T / np.where(over, p, np.float32(1.0))).astype(np.float32) * np.float32(ONE)
    assert q.dtype == np.float32
    rq = np.where(over, q.astype(np.int64), ONE).astype(np.int64)
    mq = sliding_window_view(np.concatenate([np.full(D, ONE, np.int64), rq]), W).min(axis=1)
    j = np.arange(n, dtype=np.int64)
    pm = np.minimum.accumulate(mq - j * step) if n else mq
    eq = np.minimum(ONE + (j + 1) * step, pm + j * step)
    S = sliding_window_view(np.concatenate([np.full(D, ONE, np.int64), eq]), W).sum(axis=1).astype(np.uint64)
    g = S.astype(np.float32) / np.float32(W * ONE)
    ud = np.concatenate([np.zeros((D, 2), np.float32), u])[:n]
    y = (ud * g[:, None]).astype(np.float32)
    hi, lo = y > T, y < -T
    y = np.where(hi, T, np.where(lo, -T, y)).astype(np.float32)
    return {"y": y, "u": u, "rq": rq, "mq": mq, "eq": eq, "S": S, "g": g, "frames": frames, "nonfinite": nonfinite, "limited": int((S < np.uint64(W * ONE)).sum()),
            "clamped": [int((hi | lo)[:, r].sum()) for r in range(2)], "min_gain": np.float32(g.min()) if n else np.float32(1.0),
            "eq_last": ONE if flush or n == 0 else int(eq[-1])}


# ---- signals ------------------------------------------------------------------------------------------------------------------------

def exact_at(T, gain) -> np.float32:
    """an x whose product with gain is T, where fp32 has one (else the nearest below)"""
    T, gain = np.float32(T), np.float32(gain)
    x = np.float32(T / gain)
    for _ in range(4):
        if np.float32(x * gain) > T:
            x = np.nextafter(x, np.float32(0.0))
    for _ in range(4):
        if np.float32(np.nextafter(x, np.float32(2.0)) * gain) <= T:
            x = np.nextafter(x, np.float32(2.0))
    return np.float32(x)


def stream_length(W: int, tile: int = 1024) -> int:
    """about three kernel tiles and 2W + 77 frames"""
    return 3 * tile + 2 * W + 77


def signal(n: int, gain: float, T, W: int, seed: int, tile: int = 1024) -> np.ndarray:
    """[n, 2] float32 for a station of gain `gain`: noise and a sine well under the ceiling after the gain; from frame 5W + 10 on bursts of
    8x amplitude, a single 50x frame, a run at exactly T and one an ulp above it, silence, denormals, +-inf and NaN; bursts across the
    tile edges behind them.  The first 5W + 10 frames are clean: a transparent stretch"""
    T = np.float32(T)
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    base = 0.05 * rng.standard_normal((n, 2)) + 0.25 * np.stack([np.sin(2 * np.pi * 1000.0 * t / FS), np.cos(2 * np.pi * 1000.0 * t / FS)], axis=1)
    x = (base * float(T) / float(gain)).astype(np.float32)
    e0 = 5 * W + 10
    at = e0
    x[at:at + 20] *= np.float32(8.0)
    at += 40 + W
    x[at] *= np.float32(50.0)
    at += 40 + W
    xt = exact_at(T, gain)
    x[at:at + 16, 0] = xt
    x[at:at + 16, 1] = -xt
    at += 16
    x[at:at + 16, 0] = np.nextafter(xt, np.float32(2.0))
    at += 16 + W
    x[at:at + 32] = 0.0
    at += 32
    x[at:at + 16] = np.float32(1e-40)
    x[at + 8:at + 16, 1] = np.float32(-3e-42)
    at += 16
    x[at, 0] = np.inf
    x[at + 3, 1] = -np.inf
    x[at + 5] = np.nan
    x[at + 9, 0] = np.float32(3e38)                                          # finite, and infinite after a gain above 1.14
    at += 16
    assert at < n
    for k in range(1, n // tile + 1):
        if k * tile - 6 > at and k * tile + 6 < n:
            x[k * tile - 6:k * tile + 6] *= np.float32(8.0)
    return x


def offsets(D: int) -> tuple:
    """frames that the GPU comparison's stations have taken before the calls under test: 0, 5 and W - 1"""
    return (0, 5, D)


def gpu_streams(D: int, tile: int = 1024) -> list:
    """the GPU comparison's three whole streams at look-ahead D: station c at GAINS[c], its offsets(D)[c] frames and then stream_length(W)"""
    W = D + 1
    return [signal(offsets(D)[c] + stream_length(W, tile), GAINS[c], ceiling(), W, seed=1000 * D + c, tile=tile) for c in range(3)]
