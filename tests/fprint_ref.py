"""The C restatement of the audio fingerprinter's arithmetic contract (tests/cpp/fprint_ref.c), built with gcc and called through
ctypes; an independent float64 definition in numpy (np.fft.rfft of the Hann-windowed frame, bands summed, bits taken); the a-priori
bound between the two; and the geometries and signals shared by tests/test_fprint_cpu.py and tests/test_gpu_fprint.py."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "fprint_ref.c"
# include/fmdemod.h fmd_fprint_status
STATUS_DTYPE = np.dtype([("frames", "<u8"), ("prints", "<u8"), ("nonfinite", "<u8"), ("fill", "<u4"), ("reserved", "<u4")])
assert STATUS_DTYPE.itemsize == 32


class Config(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("hop", C.c_int), ("n_sub", C.c_int), ("n_bands", C.c_int), ("f_min_hz", C.c_double),
                ("f_max_hz", C.c_double), ("max_input_frames", C.c_longlong), ("device", C.c_int)]


assert C.sizeof(Config) == 56


def config(fs=8000, hop=16, n_sub=4, n_bands=9, f_min_hz=250.0, f_max_hz=3500.0, n_channels=1, max_input_frames=65536, device=-1) -> Config:
    return Config(n_channels, fs, hop, n_sub, n_bands, f_min_hz, f_max_hz, max_input_frames, device)


def config_fields(c) -> dict:
    """every field of a Config-shaped structure by name (the library's FprintConfig has the same names)"""
    return {k: getattr(c, k) for k, _ in Config._fields_}


# the smallest geometry where every piece is live: bin edges 2, 3, 4, 5, 6, 9, 12, 16, 21, 28, K = 28 (the padding to 32 is live)
SMALL = dict(fs=8000, hop=16, n_sub=4, n_bands=9, f_min_hz=250.0, f_max_hz=3500.0)
SMALL_EDGES = [2, 3, 4, 5, 6, 9, 12, 16, 21, 28]
DEFAULT_32K = dict(fs=32000, hop=368, n_sub=32, n_bands=33, f_min_hz=300.0, f_max_hz=2000.0)


class Channel:
    """one station of the restatement: process(x [n, 2] float32) as often as wanted -> (words [T] uint32, energies [T, B]); status()"""

    def __init__(self, ref, cfg: Config):
        self.lib, self.cfg = ref.lib, cfg
        self.h = self.lib.fprint_ref_create(C.byref(cfg))
        if not self.h:
            raise ValueError("invalid configuration or design")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.fprint_ref_destroy(self.h)
            self.h = None

    def process(self, x):
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype == np.float32
        cap = (x.shape[0] + self.cfg.hop - 1) // self.cfg.hop
        out = np.zeros(max(cap, 1), np.uint32)
        en = np.zeros((max(cap, 1), self.cfg.n_bands), np.float32)
        k = self.lib.fprint_ref_process(self.h, x.ctypes.data_as(C.c_void_p), x.shape[0], out.ctypes.data_as(C.c_void_p), en.ctypes.data_as(C.c_void_p), cap)
        assert k >= 0, "more words than fmd_fprint_max_prints"
        return out[:k].copy(), en[:k].copy()

    def reset(self):
        self.lib.fprint_ref_reset(self.h)

    def status(self) -> np.ndarray:
        st = np.zeros(1, STATUS_DTYPE)
        self.lib.fprint_ref_get_status(self.h, st.ctypes.data_as(C.c_void_p))
        return st


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def channel(self, cfg: Config) -> Channel:
        return Channel(self, cfg)

    def run(self, cfg: Config, x):
        """a fresh station fed x [n, 2] in one piece: (words, energies)"""
        return self.channel(cfg).process(x)

    def check(self, cfg: Config) -> int:
        return self.lib.fprint_ref_check(C.byref(cfg))

    def default_config(self, fs: int):
        c = Config()
        return c if self.lib.fprint_ref_default_config(int(fs), C.byref(c)) == 0 else None

    def bins(self, cfg: Config) -> int:
        return self.lib.fprint_ref_bins(C.byref(cfg))

    def design(self, cfg: Config):
        """(bc [H, K], bs [H, K], wc [R], ws [R], edges [B + 1], K, first_bin)"""
        K = self.bins(cfg)
        assert K > 0
        bc, bs = (np.zeros((cfg.hop, K), np.float32) for _ in range(2))
        wc, ws = (np.zeros(cfg.n_sub, np.float32) for _ in range(2))
        edges = np.zeros(cfg.n_bands + 1, np.int32)
        k, f = C.c_int(), C.c_int()
        assert self.lib.fprint_ref_design(C.byref(cfg), *(a.ctypes.data_as(C.c_void_p) for a in (bc, bs, wc, ws, edges)), C.byref(k), C.byref(f)) == 0
        return bc, bs, wc, ws, edges, k.value, f.value

    def max_prints(self, hop: int, n: int) -> int:
        return self.lib.fprint_ref_max_prints(int(hop), int(n))

    def prints(self, f: int, hop: int, n_sub: int) -> int:
        return self.lib.fprint_ref_prints(int(f), int(hop), int(n_sub))


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libfprint_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    P = C.POINTER(Config)
    lib.fprint_ref_check.argtypes = [P]
    lib.fprint_ref_default_config.argtypes = [C.c_int, P]
    lib.fprint_ref_bins.argtypes = [P]
    lib.fprint_ref_max_prints.argtypes = [C.c_int, C.c_longlong]
    lib.fprint_ref_max_prints.restype = C.c_longlong
    lib.fprint_ref_prints.argtypes = [C.c_ulonglong, C.c_int, C.c_int]
    lib.fprint_ref_prints.restype = C.c_ulonglong
    lib.fprint_ref_design.argtypes = [P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.fprint_ref_create.argtypes = [P]
    lib.fprint_ref_create.restype = C.c_void_p
    lib.fprint_ref_destroy.argtypes = [C.c_void_p]
    lib.fprint_ref_destroy.restype = None
    lib.fprint_ref_reset.argtypes = [C.c_void_p]
    lib.fprint_ref_reset.restype = None
    lib.fprint_ref_get_status.argtypes = [C.c_void_p, C.c_void_p]
    lib.fprint_ref_get_status.restype = None
    lib.fprint_ref_process.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int]
    return Ref(lib)


def bits(a) -> np.ndarray:
    """a float32 array as its integer view (rows compare bit for bit, NaNs and signed zeros included)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the float64 definition -----------------------------------------------------------------------------------------------------

def model_edges(cfg) -> np.ndarray:
    N = cfg.n_sub * cfg.hop
    f = cfg.f_min_hz * (cfg.f_max_hz / cfg.f_min_hz) ** (np.arange(cfg.n_bands + 1) / cfg.n_bands)
    return np.floor(f * N / cfg.fs + 0.5).astype(np.int64)


def model_frames(cfg, x: np.ndarray):
    """x [n, 2] float32 -> (X [T, N / 2 + 1] complex128: np.fft.rfft of the Hann-windowed frames, m [n] float64)"""
    H, N = cfg.hop, cfg.n_sub * cfg.hop
    m = 0.5 * (x[:, 0].astype(np.float64) + x[:, 1].astype(np.float64))
    T = 0 if m.size < N else (m.size - N) // H + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    fr = np.lib.stride_tricks.sliding_window_view(m, N)[::H][:T] if T else np.zeros((0, N))
    return np.fft.rfft(fr * w[None, :], axis=1), m


def model_energy(cfg, x: np.ndarray) -> np.ndarray:
    """[T, B] float64 band energies of every frame"""
    X, _ = model_frames(cfg, x)
    e = model_edges(cfg)
    P = np.abs(X) ** 2
    return np.stack([P[:, e[b]:e[b + 1]].sum(axis=1) for b in range(cfg.n_bands)], axis=1)


def words_of_energy(E: np.ndarray) -> np.ndarray:
    """[T, B] energies -> [T - 1] uint32 words: bit b of word t is (E_t[b] - E_t[b+1]) - (E_t-1[b] - E_t-1[b+1]) > 0 at position 31 - b"""
    d = E[:, :-1] - E[:, 1:]
    dd = d[1:] - d[:-1]
    w = np.zeros(dd.shape[0], np.uint32)
    for b in range(dd.shape[1]):
        w |= (dd[:, b] > 0).astype(np.uint32) << np.uint32(31 - b)
    return w


def model_words(cfg, x: np.ndarray) -> np.ndarray:
    return words_of_energy(model_energy(cfg, x))


def ber(a, b, n_bits: int) -> float:
    """bit error rate over the top n_bits of two equally long runs of words"""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    assert a.shape == b.shape and a.size
    x = (a ^ b) >> np.uint32(32 - n_bits)
    return float(np.unpackbits(np.ascontiguousarray(x).view(np.uint8)).sum()) / (a.size * n_bits)


def apriori_bound(cfg, x: np.ndarray) -> np.ndarray:
    """[T, B]: the bound on |E32 - E64| of the contract's fp32 chains, derived, not measured, to first order in u = 2^-24 with the
    second-order term of the power kept.  Per frame, with S = sum over its N samples of |m| and S_j the same over sub-block j:
      sub-block   a chain of H fmaf steps behind one rounding of m and one of the basis entry errs by at most (H + 2) u S_j in Sr and in
                  Si alike;
      frame       the chain of 2 R fmaf steps over the R spectra, each twiddle rounded once, adds (2 R + 1) u sum_j (|Sr_j| + |Si_j|)
                  <= (2 R + 1) u 2 S, and carries the sub-blocks' errors with weight |wc| + |ws| <= sqrt(2): together
                  e_X = (sqrt(2) (H + 2) + 2 (2 R + 1)) u S bounds the error of re X_k and of im X_k at every bin;
      window      Xw = X_k / 2 - (X_k-1 + X_k+1) / 4 carries e_X with weight 1/2 + 1/4 + 1/4 = 1 and adds three roundings of values
                  no larger than |X| <= S:  e_W = e_X + 3 u S -- the three-tap window's term, proportional to u sum |m| through
                  the neighbouring bins, where the float64 definition's windowed frame has |Xw| far below S;
      power       |Xw32|^2 - |Xw|^2 <= 2 sqrt(2) |Xw| e_W + 2 e_W^2, plus two roundings: 2 u |Xw|^2;
      band        a sum of n_b non-negative terms in ascending k: (n_b - 1) u times the sum.
    The bound of band b is  sum_k (2 sqrt(2) |Xw_k| e_W + 2 e_W^2) + (n_b + 1) u sum_k (|Xw_k|^2 + 2 sqrt(2) |Xw_k| e_W + 2 e_W^2)."""
    X, m = model_frames(cfg, x)
    H, R = cfg.hop, cfg.n_sub
    N = H * R
    u = 2.0 ** -24
    T = X.shape[0]
    S = np.lib.stride_tricks.sliding_window_view(np.abs(m), N)[::H][:T].sum(axis=1) if T else np.zeros(0)
    eW = ((math.sqrt(2.0) * (H + 2) + 2.0 * (2 * R + 1)) * u * S + 3.0 * u * S)[:, None]
    A = np.abs(X)
    d = 2.0 * math.sqrt(2.0) * A * eW + 2.0 * eW * eW
    e = model_edges(cfg)
    out = np.zeros((T, cfg.n_bands))
    for b in range(cfg.n_bands):
        nb = int(e[b + 1] - e[b])
        out[:, b] = d[:, e[b]:e[b + 1]].sum(axis=1) + (nb + 1) * u * (A[:, e[b]:e[b + 1]] ** 2 + d[:, e[b]:e[b + 1]]).sum(axis=1)
    return out


# ---- signals --------------------------------------------------------------------------------------------------------------------

def programme(fs: int, n: int, seed: int, scale: float = 1.0, spread: float = 0.0) -> np.ndarray:
    """[n, 2] float32: a programme-like signal.  Notes of 0.12 ... 0.5 s, each three partials of a fundamental drawn between 200 and
    1200 Hz under a decaying envelope, over low-pass-like noise at -30 dB; the rails differ by `spread` of an independent copy"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / fs
    y = np.zeros(n)
    at = 0
    while at < n:
        ln = int(fs * rng.uniform(0.12, 0.5))
        f0 = 200.0 * 6.0 ** rng.uniform()
        seg = slice(at, min(n, at + ln))
        tt = t[seg] - t[at]
        env = np.exp(-tt * rng.uniform(2.0, 9.0)) * np.minimum(1.0, tt * 200.0)
        ph = rng.uniform(0, 2 * np.pi, 3)
        y[seg] += env * (np.sin(2 * np.pi * f0 * tt + ph[0]) + 0.5 * np.sin(2 * np.pi * 2 * f0 * tt + ph[1]) + 0.3 * np.sin(2 * np.pi * 3 * f0 * tt + ph[2]))
        at += ln
    noise = np.cumsum(rng.standard_normal(n))
    noise -= np.convolve(noise, np.ones(64) / 64.0, mode="same")
    y = 0.2 * y + 0.03 * noise / (np.std(noise) + 1e-30)
    side = spread * 0.05 * rng.standard_normal(n)
    return (scale * np.stack([y + side, y - side], axis=1)).astype(np.float32)


def signal(kind: str, fs: int, n: int, seed: int = 20261020, scale: float = 1.0) -> np.ndarray:
    """[n, 2] float32.  noise: Gaussian at -20 dB a rail, half of it common to both; tone: 1 kHz at -12 dBFS in both rails; programme: as
    above; silence: zeros"""
    rng = np.random.default_rng(seed)
    n1, n2 = rng.standard_normal(n), rng.standard_normal(n)
    t = np.arange(n, dtype=np.float64) / fs
    tone = 0.25 * np.sin(2.0 * np.pi * 1000.0 * t + 0.3)
    if kind == "noise":
        x = np.stack([0.1 * n1, 0.1 * (0.6 * n1 + 0.8 * n2)], axis=1)
    elif kind == "tone":
        x = np.stack([tone, tone], axis=1)
    elif kind == "programme":
        return programme(fs, n, seed, scale, 0.3)
    elif kind == "silence":
        x = np.zeros((n, 2))
    else:
        raise ValueError(kind)
    return (scale * x).astype(np.float32)


def mixed_signal(fs: int, n: int, order, seed: int, scale: float) -> np.ndarray:
    """[n, 2] float32: the kinds of `order` one after the other in equal parts"""
    part = -(-n // len(order))
    return np.concatenate([signal(k, fs, part, seed + i, scale) for i, k in enumerate(order)])[:n]
