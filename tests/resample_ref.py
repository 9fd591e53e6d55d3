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


POLY_SRC = SRC.parent / "resample_poly_ref.c"

# The polyphase cases of test_resample_cpu.py and test_gpu_resample_poly.py: (fs_in, fs_out, taps_per_phase asked for) -> the (L, M, T, tile)
# the library must run them with, as literals (test_resample_cpu.py asserts them against fmd_resampler_design and poly_tile)
POLY_CASES = {
    (32000, 48000, 0): (3, 2, 32, 256),
    (32000, 44100, 0): (441, 320, 32, 256),
    (32000, 22050, 0): (441, 640, 64, 256),
    (32000, 16000, 0): (1, 2, 64, 256),
    (32000, 8000, 0): (1, 4, 128, 256),
    (32000, 4000, 0): (1, 8, 256, 128),
    (32000, 192000, 0): (6, 1, 32, 256),
    (32000, 1000, 256): (1, 32, 256, 32),
    (32000, 48000, 8): (3, 2, 8, 256),
    (32000, 48000, 256): (3, 2, 256, 256),
    (48000, 44100, 0): (147, 160, 64, 256),
}


def poly_count(pos: int, k: int, L: int, M: int) -> int:
    """outputs of a call of k frames at input position pos: ceil((pos + k) L / M) - ceil(pos L / M)"""
    return -(-(pos + k) * L // M) - -(-pos * L // M)


def poly_three_calls(L: int, M: int, tile: int) -> list:
    """Input lengths of three consecutive calls from position 0 that emit 2 tile + 17 frames (two full tiles and a ragged third), one tile,
    and 37 (fewer than a wavefront).  An up-sampler's count moves in steps of up to ceil(L / M), so a target it cannot hit exactly becomes
    the next count above it: the first call is lengthened frame by frame while that lets the second hit one tile exactly."""
    def shortest(pos, target):
        k = 0
        while poly_count(pos, k, L, M) < target:
            k += 1
        return k
    best = None
    for extra in range(M + 1):
        k1 = shortest(0, 2 * tile + 17) + extra
        k2 = shortest(k1, tile)
        calls = [k1, k2, shortest(k1 + k2, 37)]
        if best is None:
            best = calls
        if poly_count(0, k1, L, M) < 3 * tile and poly_count(k1, k2, L, M) == tile:
            return calls
    return best


def poly_call_shapes(T: int) -> list:
    """the call lengths that walk a live history (after one call of 3 T frames): shorter than, equal to and longer than the T - 1 frames kept"""
    return [1, 1, 1, 0, 2, T - 2, T - 1, T, T + 1, 1, 5 * T + 3, 1, 1]


def noise_and_tone(n_channels: int, n: int, seed: int, fs_in: int = 32000) -> np.ndarray:
    """[C, n, 2] float32: white noise at 0.3 RMS, seeded per channel, plus a small tone whose frequency differs per channel and whose
    phase differs per rail"""
    t = np.arange(n) / fs_in
    x = np.empty((n_channels, n, 2), np.float32)
    for c in range(n_channels):
        rng = np.random.default_rng(1000 * seed + c)
        for r in range(2):
            x[c, :, r] = 0.3 * rng.standard_normal(n) + 0.1 * np.sin(2 * np.pi * (400.0 + 37.0 * c) * t + 0.7 * r)
    return x


def poly_tile(L: int, M: int, T: int) -> int:
    """output frames per workgroup of the polyphase kernel: 256, halved while the staged span (tile - 1) M / L + T + 1 exceeds 2048 frames
    (DESIGN.md "Audio resampler"); re-derived here so that a test meant for a small tile can assert that it has one"""
    tile = 256
    while tile > 1 and (tile - 1) * M // L + T + 1 > 2048:
        tile //= 2
    return tile


def build_poly(tmp_dir: Path):
    """The C restatement of the polyphase method (tests/cpp/resample_poly_ref.c).  Returns a class: PolyRef(C, L, M, taps [T, L]) with
    output_frames(n), process(x [C, n, 2]) -> [C, n_out, 2] float32, reset(channel), counters(); PolyRef.pcm16(y) -> (int16, unspecified mask)."""
    so = Path(tmp_dir) / "libresample_poly_ref.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(POLY_SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.poly_ref_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.poly_ref_create.restype = C.c_void_p
    lib.poly_ref_destroy.argtypes = [C.c_void_p]
    lib.poly_ref_reset.argtypes = [C.c_void_p, C.c_int]
    lib.poly_ref_output_frames.argtypes = [C.c_void_p, C.c_longlong]
    lib.poly_ref_output_frames.restype = C.c_longlong
    lib.poly_ref_process.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong]
    lib.poly_ref_process.restype = C.c_longlong
    lib.poly_ref_counters.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.poly_ref_pcm16.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]

    class PolyRef:
        def __init__(self, n_channels: int, L: int, M: int, taps: np.ndarray):
            taps = np.ascontiguousarray(taps, np.float32)
            assert taps.ndim == 2 and taps.shape[1] == L
            self.C, self.L, self.M, self.T = n_channels, L, M, taps.shape[0]
            self.h = lib.poly_ref_create(n_channels, L, M, self.T, taps.ctypes.data_as(C.c_void_p))

        def __del__(self):
            if getattr(self, "h", None):
                lib.poly_ref_destroy(self.h)
                self.h = None

        def output_frames(self, n_in: int) -> int:
            return lib.poly_ref_output_frames(self.h, n_in)

        def counters(self):
            n, o = C.c_longlong(0), C.c_longlong(0)
            lib.poly_ref_counters(self.h, C.byref(n), C.byref(o))
            return n.value, o.value

        def reset(self, channel: int = -1):
            lib.poly_ref_reset(self.h, channel)

        def process(self, x: np.ndarray) -> np.ndarray:
            x = np.ascontiguousarray(x, np.float32)
            assert x.ndim == 3 and x.shape[0] == self.C and x.shape[2] == 2
            n = x.shape[1]
            want = self.output_frames(n)
            y = np.zeros((self.C, max(want, 1), 2), np.float32)
            got = lib.poly_ref_process(self.h, x.ctypes.data_as(C.c_void_p), max(n, 1), n, y.ctypes.data_as(C.c_void_p), y.shape[1])
            assert got == want
            return y[:, :got].copy()

        @staticmethod
        def pcm16(y: np.ndarray):
            """(int16 like y, bool mask of the values the definition leaves unspecified: NaN, +-inf, |y * 31128.65| >= 2^31)"""
            y = np.ascontiguousarray(y, np.float32)
            out = np.zeros(y.shape, np.int16)
            un = np.zeros(y.shape, np.uint8)
            lib.poly_ref_pcm16(y.ctypes.data_as(C.c_void_p), y.size, out.ctypes.data_as(C.c_void_p), un.ctypes.data_as(C.c_void_p))
            return out, un.astype(bool)

    return PolyRef


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
