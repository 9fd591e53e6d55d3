"""The C restatement of the log-mel front end's arithmetic contract (tests/cpp/logmel_ref.c), built with gcc and called through
ctypes; an independent float64 definition in numpy (np.fft.rfft and the formulas of include/fmdemod.h); the a-priori bound between the
two; and the geometries and signals shared by tests/test_logmel_cpu.py and tests/test_gpu_logmel.py."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "logmel_ref.c"
# include/fmdemod.h fmd_logmel_status
STATUS_DTYPE = np.dtype([("frames", "<u8"), ("spectra", "<u8"), ("nonfinite", "<u8"), ("fill", "<u4"), ("reserved", "<u4")])
assert STATUS_DTYPE.itemsize == 32
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


class Config(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("win", C.c_int), ("hop", C.c_int), ("n_mels", C.c_int), ("f_min_hz", C.c_double),
                ("f_max_hz", C.c_double), ("mel_scale", C.c_int), ("out_mode", C.c_int), ("log_floor", C.c_float), ("max_input_frames", C.c_longlong),
                ("device", C.c_int)]


assert C.sizeof(Config) == 72


def config(fs=8000, win=64, hop=16, n_mels=8, f_min_hz=0.0, f_max_hz=None, mel_scale=0, out_mode=1, log_floor=1e-10, n_channels=1,
           max_input_frames=65536, device=-1) -> Config:
    return Config(n_channels, fs, win, hop, n_mels, f_min_hz, min(8000.0, fs / 2) if f_max_hz is None else f_max_hz, mel_scale, out_mode, log_floor,
                  max_input_frames, device)


def config_fields(c) -> dict:
    """every field of a Config-shaped structure by name (the library's LogmelConfig has the same names)"""
    return {k: getattr(c, k) for k, _ in Config._fields_}


# the five geometries of the float64 check (none has an empty band), by name
GEOMETRIES = {
    "32k": dict(fs=32000, win=800, hop=320, n_mels=80),
    "16k": dict(fs=16000, win=400, hop=160, n_mels=80),
    "48k": dict(fs=48000, win=1200, hop=480, n_mels=80),
    "8k": dict(fs=8000, win=64, hop=16, n_mels=8),
    "8k_htk": dict(fs=8000, win=64, hop=24, n_mels=8, mel_scale=1, f_min_hz=100.0, f_max_hz=3000.0),
}


class Channel:
    """one station of the restatement: process(x [n, 2] float32) as often as wanted -> the completed rows [T, n_mels]; status()"""

    def __init__(self, ref, cfg: Config):
        self.lib, self.cfg = ref.lib, cfg
        self.h = self.lib.logmel_ref_create(C.byref(cfg))
        if not self.h:
            raise ValueError("invalid configuration")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.logmel_ref_destroy(self.h)
            self.h = None

    def process(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype == np.float32
        cap = (x.shape[0] + self.cfg.hop - 1) // self.cfg.hop
        out = np.zeros((max(cap, 1), self.cfg.n_mels), np.float32)
        rows = self.lib.logmel_ref_process(self.h, x.ctypes.data_as(C.c_void_p), x.shape[0], out.ctypes.data_as(C.c_void_p), cap)
        assert rows >= 0, "more spectral frames than fmd_logmel_max_frames"
        return out[:rows].copy()

    def reset(self):
        self.lib.logmel_ref_reset(self.h)

    def status(self) -> np.ndarray:
        st = np.zeros(1, STATUS_DTYPE)
        self.lib.logmel_ref_get_status(self.h, st.ctypes.data_as(C.c_void_p))
        return st


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def channel(self, cfg: Config) -> Channel:
        return Channel(self, cfg)

    def run(self, cfg: Config, x) -> np.ndarray:
        """a fresh station fed x [n, 2] in one piece: its rows"""
        return self.channel(cfg).process(x)

    def check(self, cfg: Config) -> int:
        return self.lib.logmel_ref_check(C.byref(cfg))

    def default_config(self, fs: int):
        c = Config()
        return c if self.lib.logmel_ref_default_config(int(fs), C.byref(c)) == 0 else None

    def bins(self, cfg: Config) -> int:
        return self.lib.logmel_ref_bins(C.byref(cfg))

    def design(self, cfg: Config):
        """(w, tc, ts, fb [n_mels, K], K, empty_bands)"""
        K = self.bins(cfg)
        assert K > 0
        w, tc, ts = (np.zeros(cfg.win, np.float32) for _ in range(3))
        fb = np.zeros((cfg.n_mels, K), np.float32)
        k, e = C.c_int(), C.c_int()
        assert self.lib.logmel_ref_design(C.byref(cfg), *(a.ctypes.data_as(C.c_void_p) for a in (w, tc, ts, fb)), C.byref(k), C.byref(e)) == 0
        return w, tc, ts, fb, k.value, e.value

    def max_frames(self, hop: int, n: int) -> int:
        return self.lib.logmel_ref_max_frames(int(hop), int(n))

    def T(self, f: int, win: int, hop: int) -> int:
        return self.lib.logmel_ref_T(int(f), int(win), int(hop))

    def flog10(self, x) -> np.ndarray:
        a = np.ascontiguousarray(x, np.float32).reshape(-1)
        out = np.zeros_like(a)
        self.lib.logmel_ref_flog10_array(a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), a.size)
        return out.reshape(np.shape(x))

    def flog10_sweep(self, first: int, last: int, stride: int):
        """(worst error in fp32 ulp against float64 log10, its argument's bits, floats) over the bit patterns first, first + stride ... last"""
        at, count = C.c_uint(), C.c_ulonglong()
        w = self.lib.logmel_ref_flog10_sweep(int(first), int(last), int(stride), C.byref(at), C.byref(count))
        return w, at.value, count.value

    def clamp(self, mel: float, floor: float) -> float:
        return self.lib.logmel_ref_clamp(mel, floor)

    def out(self, mel: float, mode: int, floor: float) -> float:
        return self.lib.logmel_ref_out(mel, int(mode), floor)

    def mel(self, f: float, scale: int) -> float:
        return self.lib.logmel_ref_mel(f, int(scale))

    def mel_inv(self, m: float, scale: int) -> float:
        return self.lib.logmel_ref_mel_inv(m, int(scale))


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "liblogmel_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    P = C.POINTER(Config)
    lib.logmel_ref_check.argtypes = [P]
    lib.logmel_ref_default_config.argtypes = [C.c_int, P]
    lib.logmel_ref_bins.argtypes = [P]
    lib.logmel_ref_max_frames.argtypes = [C.c_int, C.c_longlong]
    lib.logmel_ref_max_frames.restype = C.c_longlong
    lib.logmel_ref_T.argtypes = [C.c_ulonglong, C.c_int, C.c_int]
    lib.logmel_ref_T.restype = C.c_ulonglong
    lib.logmel_ref_design.argtypes = [P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    for fn in ("logmel_ref_mel", "logmel_ref_mel_inv"):
        getattr(lib, fn).argtypes = [C.c_double, C.c_int]
        getattr(lib, fn).restype = C.c_double
    lib.logmel_ref_flog10_array.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong]
    lib.logmel_ref_flog10_array.restype = None
    lib.logmel_ref_flog10_sweep.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)]
    lib.logmel_ref_flog10_sweep.restype = C.c_double
    lib.logmel_ref_clamp.argtypes = [C.c_float, C.c_float]
    lib.logmel_ref_clamp.restype = C.c_float
    lib.logmel_ref_out.argtypes = [C.c_float, C.c_int, C.c_float]
    lib.logmel_ref_out.restype = C.c_float
    lib.logmel_ref_create.argtypes = [P]
    lib.logmel_ref_create.restype = C.c_void_p
    lib.logmel_ref_destroy.argtypes = [C.c_void_p]
    lib.logmel_ref_destroy.restype = None
    lib.logmel_ref_reset.argtypes = [C.c_void_p]
    lib.logmel_ref_reset.restype = None
    lib.logmel_ref_get_status.argtypes = [C.c_void_p, C.c_void_p]
    lib.logmel_ref_get_status.restype = None
    lib.logmel_ref_process.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int]
    return Ref(lib)


def bits(a) -> np.ndarray:
    """a float32 array as its integer view (rows compare bit for bit, NaNs and signed zeros included)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the float64 definition -----------------------------------------------------------------------------------------------------

def model_mel(f, scale: int):
    f = np.asarray(f, np.float64)
    if scale == 1:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def model_mel_inv(m, scale: int):
    m = np.asarray(m, np.float64)
    if scale == 1:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)))


def model_bins(cfg) -> int:
    return min(cfg.win // 2, int(math.floor(cfg.f_max_hz * cfg.win / cfg.fs))) + 1


def model_filterbank(cfg) -> np.ndarray:
    """[n_mels, K] float64"""
    K = model_bins(cfg)
    mu = model_mel(cfg.f_min_hz, cfg.mel_scale) + np.arange(cfg.n_mels + 2) * (model_mel(cfg.f_max_hz, cfg.mel_scale) - model_mel(cfg.f_min_hz, cfg.mel_scale)) / (cfg.n_mels + 1)
    F = model_mel_inv(mu, cfg.mel_scale)
    fk = np.arange(K) * cfg.fs / cfg.win
    up = (fk[None, :] - F[:-2, None]) / (F[1:-1] - F[:-2])[:, None]
    down = (F[2:, None] - fk[None, :]) / (F[2:] - F[1:-1])[:, None]
    s = 2.0 / (F[2:] - F[:-2]) if cfg.mel_scale == 0 else np.ones(cfg.n_mels)
    return np.maximum(0.0, np.minimum(up, down)) * s[:, None]


def model_frames(cfg, x: np.ndarray):
    """x [n, 2] float32 -> (X [T, K] complex128 of the windowed frames, xw [T, N] float64): np.fft.rfft of w64 * m64, cut to K bins"""
    N, hop = cfg.win, cfg.hop
    m = 0.5 * (x[:, 0].astype(np.float64) + x[:, 1].astype(np.float64))
    T = 0 if m.size < N else (m.size - N) // hop + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    xw = np.stack([w * m[t * hop:t * hop + N] for t in range(T)]) if T else np.zeros((0, N))
    return np.fft.rfft(xw, axis=1)[:, :model_bins(cfg)], xw


def model_mel_power(cfg, x: np.ndarray) -> np.ndarray:
    """[T, n_mels] float64 mel powers"""
    X, _ = model_frames(cfg, x)
    return (np.abs(X) ** 2) @ model_filterbank(cfg).T


def apriori_bound(cfg, x: np.ndarray, fb32: np.ndarray) -> np.ndarray:
    """[T, n_mels]: the bound on |mel32 - mel64| of the contract's fp32 chains, derived, not measured.  With u = 2^-24 and S = sum |xw|: a
    chain of N fmaf steps behind one rounding of xw and one of the table entry errs by at most (N + 3) u S to first order in re and in
    im alike, so |X32 - X| <= E = sqrt(2) (N + 3) u S; the power then errs by 2 |X| E + E^2 plus its own two roundings, and the band's
    chain of K steps over non-negative terms by (K + 3) u times the sum of its terms' magnitudes:
    sum_k fb (2 |X_k| E + E^2) + (K + 3) u sum_k fb (|X_k|^2 + 2 |X_k| E + E^2)"""
    X, xw = model_frames(cfg, x)
    N, K = cfg.win, X.shape[1]
    u = 2.0 ** -24
    S = np.abs(xw).sum(axis=1)
    E = (math.sqrt(2.0) * (N + 3) * u * S)[:, None]
    A = np.abs(X)
    d = 2.0 * A * E + E * E
    fb = fb32.astype(np.float64)
    return d @ fb.T + (K + 3) * u * ((A * A + d) @ fb.T)


# ---- signals --------------------------------------------------------------------------------------------------------------------

def signal(kind: str, fs: int, n: int, seed: int = 20261020, scale: float = 1.0) -> np.ndarray:
    """[n, 2] float32.  noise: Gaussian at -20 dB a rail, half of it common to both; tone: 1 kHz at -12 dBFS in both rails; tone_noise:
    the tone over noise at -80 dB; silence: zeros"""
    rng = np.random.default_rng(seed)
    n1, n2 = rng.standard_normal(n), rng.standard_normal(n)
    t = np.arange(n, dtype=np.float64) / fs
    tone = 0.25 * np.sin(2.0 * np.pi * 1000.0 * t + 0.3)
    if kind == "noise":
        x = np.stack([0.1 * n1, 0.1 * (0.6 * n1 + 0.8 * n2)], axis=1)
    elif kind == "tone":
        x = np.stack([tone, tone], axis=1)
    elif kind == "tone_noise":
        x = np.stack([tone + 1e-4 * n1, tone + 1e-4 * n2], axis=1)
    elif kind == "silence":
        x = np.zeros((n, 2))
    else:
        raise ValueError(kind)
    return (scale * x).astype(np.float32)


def mixed_signal(fs: int, n: int, order, seed: int, scale: float) -> np.ndarray:
    """[n, 2] float32: the kinds of `order` one after the other in equal parts"""
    part = -(-n // len(order))
    return np.concatenate([signal(k, fs, part, seed + i, scale) for i, k in enumerate(order)])[:n]
