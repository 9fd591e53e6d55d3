"""The C restatement of the reference's audio resampler (tests/cpp/resample_ref.c), built with gcc and called through ctypes."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "resample_ref.c"


def build(tmp_dir: Path):
    so = Path(tmp_dir) / "libresample_ref.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.resample_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.resample_ref.restype = C.c_int

    def resample(x: np.ndarray, fs_out: int, fs_in: int = 32000):
        """x [n, 2] float32 -> [n_out, 2] float32, or None where the reference would index past the input"""
        x = np.ascontiguousarray(x, np.float32)
        cap = int(x.shape[0] * fs_out // fs_in) + 2
        out = np.empty((max(cap, x.shape[0]), 2), np.float32)
        n = lib.resample_ref(x.ctypes.data_as(C.c_void_p), x.shape[0], fs_in, fs_out, out.ctypes.data_as(C.c_void_p), out.shape[0])
        assert n != -2
        return None if n < 0 else out[:n].copy()
    return resample


def polyphase_f64(x: np.ndarray, taps: np.ndarray, L: int, M: int, n0: int, n1: int) -> np.ndarray:
    """y[n] = sum_t h[p + t L] x[floor(n M / L) - t] (x zero before frame 0) for n0 <= n < n1, in float64.  x [n, 2], taps [T, L]."""
    T = taps.shape[0]
    n = np.arange(n0, n1, dtype=np.int64)
    m = (n * M) // L
    p = (n * M) % L
    xp = np.concatenate([np.zeros((T - 1, 2)), np.asarray(x, np.float64)])
    idx = m[:, None] - np.arange(T)[None, :] + (T - 1)          # [n, T]
    h = taps.astype(np.float64)[np.arange(T)[None, :], p[:, None]]  # [n, T]
    return np.einsum("nt,ntc->nc", h, xp[idx])
